// warp.hip -- homography grid, bilinear grid_sample and the fused fine-flow composition.
//   warp_grid     kornia HomographyWarper.warp_grid   (quick_start/align2images.py:61,65)
//   grid_sample   F.grid_sample(bilinear, zeros)      (quick_start/align2images.py:66,95,97;
//                                                       evaluation/evalHpatch/evaluation.py:25,45)
//   compose_flow  F.interpolate + grid add (+clamp) + grid_sample of the coarse grid (+ in-bounds mask)
//                                                      (quick_start/align2images.py:92-95;
//                                                       evaluation/evalHpatch/evaluation.py:40-45,51)
// All HBM-bound gathers: one thread per output pixel, consecutive threads along W; channels looped in
// the thread so the 4 corner offsets / weights are computed once per pixel.
#include "common.h"
#include "group.h"
#include "linspace.h"
#include "assemble_pixel.h"
#include <math.h>

namespace {

inline int grid_for(long long total, int block) {
    long long g = (total + block - 1) / block;
    const long long cap = 256LL * 32;
    return (int)(g < cap ? g : cap);
}

// Argument blocks of the three fine-stage kernels.  Each kernel body is a typed device function of (arguments, the problem's own
// block index bx, the problem's own grid gx): the single launch passes blockIdx.x / gridDim.x, the grouped launch (group.h) passes
// blockIdx.x / the grid the problem recorded -- the grid-stride loops stride by THAT, not by the launch's gridDim.x, which is the
// largest problem's.
struct WarpGridArgs { const float* Hm; float* grid; long long total; int h, w; };
struct GridSampleArgs { const float* in; const float* grid; float* out; long long NP; int C, Hi, Wi, Ho, Wo, align; };
struct ComposeFlowArgs {
    const float* flowDown; const float* coarse; float* flow12; float* inb; float* flowUp;
    long long NP; int hd, wd, Hc, Wc, H, W; float sh, sw; int clampf;
};

__device__ __forceinline__ void warp_grid_body(const WarpGridArgs& a, const unsigned bx, const unsigned gx) {
    const float* __restrict__ Hm = a.Hm;
    float* __restrict__ grid = a.grid;
    const long long total = a.total;
    const int h = a.h, w = a.w;
    for (long long idx = (long long)bx * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gx * blockDim.x) {
        const int x = (int)(idx % w);
        const long long r = idx / w;
        const int y = (int)(r % h);
        const int b = (int)(r / h);
        const float* M = Hm + b * 9;
        const float2 o = warp_point(M, x, y, h, w);
        reinterpret_cast<float2*>(grid)[idx] = o;
    }
}

using WarpGrid = RfxFamily<WarpGridArgs, warp_grid_body, 256>;
__global__ __launch_bounds__(WarpGrid::BLOCK) void warp_grid_kernel(WarpGridArgs a) { warp_grid_body(a, blockIdx.x, gridDim.x); }

__device__ __forceinline__ void grid_sample_body(const GridSampleArgs& a, const unsigned bx, const unsigned gx) {
    const float* __restrict__ in = a.in;
    const float* __restrict__ grid = a.grid;
    float* __restrict__ out = a.out;
    const long long NP = a.NP;
    const int C = a.C, Hi = a.Hi, Wi = a.Wi, Ho = a.Ho, Wo = a.Wo, align = a.align;
    const size_t HWi = (size_t)Hi * Wi, HWo = (size_t)Ho * Wo;
    for (long long p = (long long)bx * blockDim.x + threadIdx.x; p < NP;
         p += (long long)gx * blockDim.x) {
        const long long n = p / (long long)HWo;
        const size_t px = (size_t)(p - n * (long long)HWo);
        const float2 g = reinterpret_cast<const float2*>(grid)[p];
        const Corners c = corners(g.x, g.y, Hi, Wi, align);
        const float* src = in + (size_t)n * C * HWi;
        float* dst = out + (size_t)n * C * HWo + px;
        const long long o00 = (long long)c.y0 * Wi + c.x0;
        for (int ch = 0; ch < C; ++ch) {
            const float* s = src + (size_t)ch * HWi;
            float v = 0.0f;
            if (c.m_nw) v += s[o00] * c.nw;
            if (c.m_ne) v += s[o00 + 1] * c.ne;
            if (c.m_sw) v += s[o00 + Wi] * c.sw;
            if (c.m_se) v += s[o00 + Wi + 1] * c.se;
            dst[(size_t)ch * HWo] = v;
        }
    }
}

using GridSample = RfxFamily<GridSampleArgs, grid_sample_body, 256>;
__global__ __launch_bounds__(GridSample::BLOCK) void grid_sample_kernel(GridSampleArgs a) { grid_sample_body(a, blockIdx.x, gridDim.x); }

__device__ __forceinline__ void compose_flow_body(const ComposeFlowArgs& a, const unsigned bx, const unsigned gx) {
    const float* __restrict__ flowDown = a.flowDown;
    const float* __restrict__ coarse = a.coarse;
    float* __restrict__ flow12 = a.flow12;
    float* __restrict__ inb = a.inb;
    float* __restrict__ flowUp = a.flowUp;
    const long long NP = a.NP;
    const int hd = a.hd, wd = a.wd, Hc = a.Hc, Wc = a.Wc, H = a.H, W = a.W, clampf = a.clampf;
    const float sh = a.sh, sw = a.sw;
    const size_t HW = (size_t)H * W, hw = (size_t)hd * wd, HWc = (size_t)Hc * Wc;
    for (long long p = (long long)bx * blockDim.x + threadIdx.x; p < NP;
         p += (long long)gx * blockDim.x) {
        const long long n = p / (long long)HW;
        const int px = (int)(p - n * (long long)HW);
        const int y = px / W, x = px - y * W;
        // bilinear up-sampling of the residual flow (align_corners=False)
        const float fy = src_index(sh, y), fx = src_index(sw, x);
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < hd - 1 ? 1 : 0), x1 = x0 + (x0 < wd - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
        const float* f = flowDown + (size_t)n * 2 * hw;
        float u[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float* s = f + c * hw;
            u[c] = hy * (hx * s[(size_t)y0 * wd + x0] + lx * s[(size_t)y0 * wd + x1]) +
                   ly * (hx * s[(size_t)y1 * wd + x0] + lx * s[(size_t)y1 * wd + x1]);
        }
        float gx = u[0] + rfx_lin(x, W), gy = u[1] + rfx_lin(y, H);
        if (clampf) {
            gx = fminf(fmaxf(gx, -1.0f), 1.0f);
            gy = fminf(fmaxf(gy, -1.0f), 1.0f);
        }
        if (flowUp) {
            float2 o; o.x = gx; o.y = gy;
            reinterpret_cast<float2*>(flowUp)[p] = o;
        }
        // sample the coarse grid (N,Hc,Wc,2 == 2 channels interleaved; Hc x Wc = H x W except in the KITTI driver's
        // full-resolution pass, evaluation/evalKITTI/evaluation.py:302) at (gx, gy)
        const Corners c = corners(gx, gy, Hc, Wc, 0);
        const float2* cg = reinterpret_cast<const float2*>(coarse) + (size_t)n * HWc;
        const long long o00 = (long long)c.y0 * Wc + c.x0;
        float ox = 0.f, oy = 0.f;
        if (c.m_nw) { const float2 v = cg[o00]; ox += v.x * c.nw; oy += v.y * c.nw; }
        if (c.m_ne) { const float2 v = cg[o00 + 1]; ox += v.x * c.ne; oy += v.y * c.ne; }
        if (c.m_sw) { const float2 v = cg[o00 + Wc]; ox += v.x * c.sw; oy += v.y * c.sw; }
        if (c.m_se) { const float2 v = cg[o00 + Wc + 1]; ox += v.x * c.se; oy += v.y * c.se; }
        float2 o; o.x = ox; o.y = oy;
        reinterpret_cast<float2*>(flow12)[p] = o;
        if (inb) inb[p] = (ox >= -1.0f && ox <= 1.0f && oy >= -1.0f && oy <= 1.0f) ? 1.0f : 0.0f;
    }
}

using ComposeFlow = RfxFamily<ComposeFlowArgs, compose_flow_body, 256>;
__global__ __launch_bounds__(ComposeFlow::BLOCK) void compose_flow_kernel(ComposeFlowArgs a) { compose_flow_body(a, blockIdx.x, gridDim.x); }

// Multi-homography merge of the offline flow assembly (evaluation/evalHpatch/getResults.py:48-61,
// evaluation/evalCorr/getResults.py:121-134, evaluation/evalKITTI/getResults.py:126-138): one thread per pixel walks the
// n homographies in order.  score_i = m12_i (* cyc_i) (* inb_i), multiplied left to right like the reference's
// tensor expression; pixel owner = 0 if score_0 >= th, else the first i >= 1 with score_i >= th (only if multiH), else 0.
__global__ __launch_bounds__(256) void merge_multi_h_kernel(const float* __restrict__ flow, const float* __restrict__ m12,
                                                           long long m12_stride, const float* __restrict__ cyc,
                                                           const float* __restrict__ inb, int n, long long HW, float th,
                                                           int multiH, float* __restrict__ flowG,
                                                           float* __restrict__ matchG, uint8_t* __restrict__ binary) {
    // grid-stride: grid_for() caps the grid, images above 2^21 pixels take several trips
    const int last = multiH ? n : 1;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (long long)gridDim.x * blockDim.x) {
        int best = 0;
        float mbest = 0.0f;
        bool found = false;
        for (int i = 0; i < last; ++i) {
            float v = m12[(long long)i * m12_stride + p];
            if (cyc) v = v * cyc[(long long)i * HW + p];
            if (inb) v = v * inb[(long long)i * HW + p];
            if (i == 0) mbest = v;
            if (v >= th) {
                best = i;
                mbest = v;
                found = true;
                break;
            }
        }
        const float2 f = reinterpret_cast<const float2*>(flow)[(long long)best * HW + p];
        // torch.clamp: a NaN stays a NaN (fminf / fmaxf would drop it).  A degenerate homography (z' = 0 inside the image) puts
        // one into its coarse grid, and the reference hands it on to whoever reads the flow
        float2 o;
        o.x = f.x < -1.0f ? -1.0f : (f.x > 1.0f ? 1.0f : f.x);
        o.y = f.y < -1.0f ? -1.0f : (f.y > 1.0f ? 1.0f : f.y);
        reinterpret_cast<float2*>(flowG)[p] = o;
        if (matchG) matchG[p] = mbest;
        if (binary) binary[p] = found ? 1 : 0;
    }
}

// score = match12 (* cyc) (* inb), left to right: the "match" tensor of evaluation/evalKITTI/getResults.py:120, needed
// materialised only when the host-side small-component filter (:122) sits between it and the merge.
__global__ __launch_bounds__(256) void match_score_kernel(const float* __restrict__ m12, long long m12_stride,
                                                         const float* __restrict__ cyc, const float* __restrict__ inb,
                                                         long long HW, long long total, float* __restrict__ out) {
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const long long i = q / HW, p = q - i * HW;
        float v = m12[i * m12_stride + p];
        if (cyc) v = v * cyc[q];
        if (inb) v = v * inb[q];
        out[q] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// cycle_tail: the tail of the cycle-checked PredFlowMask forms (evaluation/evalYFCC/evaluation.py:47-58, evalKITTI/evaluation.py:66-81),
// what rfx_resize_bilinear_f32(align_corners = 0) of both matchability maps -> rfx_compose_flow_f32(clamp, inb, flowUp) ->
// rfx_grid_sample_f32(up-sampled match21, flowUp) -> rfx_match_score_f32 give, per pixel, without the four full-resolution maps in
// between (both up-sampled matchabilities, flowUp, inb, the sampled cycle map).  The /8 maps are a few KB per image and stay in cache.
// Every float operation is the chain's, spelled out (__fmul_rn / __fadd_rn / fmaf) as the chain's kernels are compiled: the sums the
// compiler contracts there are the fmaf calls here, so the result does not depend on what it would contract in this body.
struct CycleTailArgs {
    const float* flowDown; const float* m12; const float* m21; const float* coarse; float* flow12; float* match;
    long long NP, m12_stride, m21_stride;    // N * H * W; floats between two images' planes of match12Down8 / match21Down8
    int hd, wd, Hc, Wc, H, W; float sh, sw;
};

__device__ __forceinline__ void cycle_tail_body(const CycleTailArgs& a, const unsigned bx, const unsigned gx_) {
    const float* __restrict__ flowDown = a.flowDown;
    const float* __restrict__ m12 = a.m12;
    const float* __restrict__ m21 = a.m21;
    const float* __restrict__ coarse = a.coarse;
    float* __restrict__ flow12 = a.flow12;
    float* __restrict__ match = a.match;
    const int hd = a.hd, wd = a.wd, Hc = a.Hc, Wc = a.Wc, H = a.H, W = a.W;
    const float sh = a.sh, sw = a.sw;
    const size_t HW = (size_t)H * W, hw = (size_t)hd * wd, HWc = (size_t)Hc * Wc;
    for (long long p = (long long)bx * blockDim.x + threadIdx.x; p < a.NP; p += (long long)gx_ * blockDim.x) {
        const long long n = p / (long long)HW;
        const int px = (int)(p - n * (long long)HW);
        const int y = px / W, x = px - y * W;
        const UpTap t = up_tap(sh, sw, y, x, hd, wd);
        // compose_flow (clamp = 1): the sampling grid, flow12, the in-bounds mask
        const float* f = flowDown + (size_t)n * 2 * hw;
        float gx = __fadd_rn(up_flow(f, t), rfx_lin(x, W)), gy = __fadd_rn(up_flow(f + hw, t), rfx_lin(y, H));
        gx = fminf(fmaxf(gx, -1.0f), 1.0f);
        gy = fminf(fmaxf(gy, -1.0f), 1.0f);
        const Corners c = corners(gx, gy, Hc, Wc, 0);
        const float2* cg = reinterpret_cast<const float2*>(coarse) + (size_t)n * HWc;
        const long long o00 = (long long)c.y0 * Wc + c.x0;
        float ox = 0.f, oy = 0.f;
        if (c.m_nw) { const float2 v = cg[o00]; ox = fmaf(v.x, c.nw, ox); oy = fmaf(v.y, c.nw, oy); }
        if (c.m_ne) { const float2 v = cg[o00 + 1]; ox = fmaf(v.x, c.ne, ox); oy = fmaf(v.y, c.ne, oy); }
        if (c.m_sw) { const float2 v = cg[o00 + Wc]; ox = fmaf(v.x, c.sw, ox); oy = fmaf(v.y, c.sw, oy); }
        if (c.m_se) { const float2 v = cg[o00 + Wc + 1]; ox = fmaf(v.x, c.se, ox); oy = fmaf(v.y, c.se, oy); }
        float2 o; o.x = ox; o.y = oy;
        reinterpret_cast<float2*>(flow12)[p] = o;
        const float inb = (ox >= -1.0f && ox <= 1.0f && oy >= -1.0f && oy <= 1.0f) ? 1.0f : 0.0f;
        // resize_bilinear of match12Down8 at the pixel
        const float v12 = up_resize(m12 + n * a.m12_stride, t);
        // grid_sample of the up-sampled match21 (H x W) at (gx, gy): each tap is the resize expression at that tap's integer pixel
        const Corners k = corners(gx, gy, H, W, 0);
        const float* s21 = m21 + n * a.m21_stride;
        float cyc = 0.0f;
        if (k.m_nw) cyc = fmaf(up_resize(s21, up_tap(sh, sw, k.y0, k.x0, hd, wd)), k.nw, cyc);
        if (k.m_ne) cyc = fmaf(up_resize(s21, up_tap(sh, sw, k.y0, k.x0 + 1, hd, wd)), k.ne, cyc);
        if (k.m_sw) cyc = fmaf(up_resize(s21, up_tap(sh, sw, k.y0 + 1, k.x0, hd, wd)), k.sw, cyc);
        if (k.m_se) cyc = fmaf(up_resize(s21, up_tap(sh, sw, k.y0 + 1, k.x0 + 1, hd, wd)), k.se, cyc);
        // match_score: (match12 * cycle) * in-bounds, left to right
        match[p] = __fmul_rn(__fmul_rn(v12, cyc), inb);
    }
}

using CycleTail = RfxFamily<CycleTailArgs, cycle_tail_body, 256>;
__global__ __launch_bounds__(CycleTail::BLOCK) void cycle_tail_kernel(CycleTailArgs a) { cycle_tail_body(a, blockIdx.x, gridDim.x); }

// ---------------------------------------------------------------------------------------------------------------------------------
// assemble_records: the offline flow assembly (evaluation/evalHpatch/getResults.py:16-63, evalCorr/getResults.py:78-136,
// evalYFCC/getResults.py:150-190) of EVERY pair of a batch straight from the drivers' result records -- what, per pair,
// rfx_warp_grid_f32 -> rfx_compose_flow_f32(clamp, inb[, flowUp]) -> rfx_resize_bilinear_f32 [-> rfx_grid_sample_f32] ->
// rfx_merge_multi_h_f32 give on the record's first nbH entries, bit for bit, in one launch: nbH is read here, nothing of size (n,H,W)
// is stored.  blockIdx.y = the pair, blockIdx.x strides over the pair's own H x W pixels; a thread walks the homographies in the
// merge's order and stops at the owner, so homography i >= 1 is evaluated only at the pixels that reach it.  The coarse grid of a
// homography is not stored either: a tap of its bilinear sample is warp_grid_body's expression at the tap's integer pixel.
// Float operations are spelled out as in cycle_tail_body.
struct AssembleRecArgs {
    const float* rec; const long long* table; const uint8_t* bg; float* flowG; float* matchG; uint8_t* binary;
    long long rec_elems, total_px;           // floats in rec; pixels in each of the packed outputs (and in bg)
    int width, max_h, off_H, off_flow, multiH, cycle; float th;
};

__global__ __launch_bounds__(256) void assemble_records_kernel(AssembleRecArgs a) {
    // row blockIdx.y of the table, checked (assemble_pixel.h): a row that does not describe a record inside rec and a map inside the
    // outputs is skipped, no read or write leaves the buffers
    const RecPair k = rec_pair(a.rec, a.rec_elems, a.table, blockIdx.y, a.width, a.max_h, a.off_H, a.off_flow, a.multiH, a.total_px);
    if (!k.ok) return;
    const int W = k.W, HW = k.HW;
    const uint8_t* __restrict__ bg = a.bg ? a.bg + k.out_off : nullptr;
    float2* __restrict__ flowG = reinterpret_cast<float2*>(a.flowG) + k.out_off;
    float* __restrict__ matchG = a.matchG + k.out_off;
    uint8_t* __restrict__ binary = a.binary + k.out_off;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += (long long)gridDim.x * blockDim.x) {
        const int p = (int)q;
        const int y = p / W, x = p - y * W;
        const PixelResult r = assemble_pixel(k, y, x, a.cycle, a.th);
        flowG[p] = r.flow;
        matchG[p] = r.match;
        binary[p] = (r.found && (!bg || bg[p] != 0)) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// assemble_kitti_records: the KITTI form of the assembly above (evaluation/evalKITTI/getResults.py:95-141, getFlow_all) from records
// that carry the half-resolution flowD2 -- per pair what rfx_warp_grid_f32 -> rfx_compose_flow_f32(flowD2, clamp) ->
// rfx_compose_flow_f32(flowDown8, clamp, inb, flowUp) -> rfx_resize_bilinear_f32 -> rfx_grid_sample_f32 -> [rfx_match_score_f32 ->
// rfx_remove_small_cc_f32 ->] rfx_merge_multi_h_f32 give on the record's first nbH entries, bit for bit.  The flow is a two-level
// composition: a tap of the fine flow's bilinear sample is the d2 flow at that tap's integer pixel, itself a four-tap sample of the
// homography grid, so a pixel costs up to 16 warp_points per homography and neither d2, flowUp, inb nor an up-sampled map is stored.
// Row blockIdx.y of the (B,12) table: row offset in rec | h8 | w8 | off_match | off_d2 | hd2 | wd2 | H | W | offset of the pair's
// pixels in the outputs | element offset of the pair's score map 0 | max_area of the component filter.
struct KittiRecArgs {
    const float* rec; const long long* table; float* scores; int32_t* dims; float* flowG; float* matchG; uint8_t* binary;
    long long rec_elems, total_px, score_base, score_elems;   // floats in rec; pixels in each packed output; the score buffer holds
                                                              // the elements [score_base, score_base + score_elems) of the batch's
    int width, max_h, off_H, off_flow, multiH; float th;
};

constexpr int KITTI_COLS = 12;

// one pair of the table, checked: nothing is read or written for a row with ok == false
struct KittiPair {
    const float* Hm; const float* flowDown; const float* matchDown; const float* flowD2;
    long long out_off, score_off;            // score_off: relative to the score buffer
    int hd, wd, hd2, wd2, H, W, HW, nb, last, max_area;
    float sh8, sw8, sh2, sw2;
    bool ok;
};

__device__ __forceinline__ KittiPair kitti_pair(const KittiRecArgs& a, const int b, const bool need_scores) {
    const long long* __restrict__ T = a.table + (long long)b * KITTI_COLS;
    const long long row_off = T[0], h8l = T[1], w8l = T[2], off_match = T[3], off_d2 = T[4], hd2l = T[5], wd2l = T[6], Hl = T[7],
                    Wl = T[8], out_off = T[9], score_off = T[10] - a.score_base, area = T[11];
    KittiPair k;
    k.ok = false;
    if (row_off < 0 || row_off + a.width > a.rec_elems || h8l <= 0 || w8l <= 0 || h8l > a.width || w8l > a.width || h8l * w8l > a.width ||
        hd2l <= 0 || wd2l <= 0 || hd2l > a.width || wd2l > a.width || hd2l * wd2l > a.width || Hl <= 0 || Wl <= 0 ||
        Hl > 0x7fffffffLL || Wl > 0x7fffffffLL || Hl * Wl > 0x7fffffffLL || area < 0 || area > 0x7fffffffLL)
        return k;
    const long long n8 = 2 * h8l * w8l * a.max_h, n2 = 2 * hd2l * wd2l * a.max_h, HWl = Hl * Wl;
    if (off_match < a.off_flow + n8 || off_d2 < off_match + n8 || off_d2 + n2 > a.width || out_off < 0 || out_off + HWl > a.total_px)
        return k;
    if (need_scores && (score_off < 0 || score_off + HWl * a.max_h > a.score_elems)) return k;
    const float* __restrict__ row = a.rec + row_off;
    k.Hm = row + a.off_H; k.flowDown = row + a.off_flow; k.matchDown = row + off_match; k.flowD2 = row + off_d2;
    k.out_off = out_off; k.score_off = score_off;
    k.hd = (int)h8l; k.wd = (int)w8l; k.hd2 = (int)hd2l; k.wd2 = (int)wd2l; k.H = (int)Hl; k.W = (int)Wl; k.HW = (int)HWl;
    k.max_area = (int)area;
    const float nf = row[0];                                   // nbH, a small integer held as a float
    k.nb = nf >= 1.0f ? (nf < (float)a.max_h ? (int)nf : a.max_h) : 0;
    k.last = a.multiH ? k.nb : (k.nb < 1 ? k.nb : 1);
    k.sh8 = (float)k.hd / (float)k.H; k.sw8 = (float)k.wd / (float)k.W;
    k.sh2 = (float)k.hd2 / (float)k.H; k.sw2 = (float)k.wd2 / (float)k.W;
    k.ok = true;
    return k;
}

// level 1: d2 = compose_flow(flowD2_i, warp_grid(H_i), clamp) at the integer pixel (x, y) of the H x W grid
__device__ __forceinline__ float2 kitti_d2_point(const KittiPair& k, const int i, const int x, const int y) {
    const int hw2 = k.hd2 * k.wd2, H = k.H, W = k.W;
    const UpTap t = up_tap(k.sh2, k.sw2, y, x, k.hd2, k.wd2);
    const float* f = k.flowD2 + (size_t)i * 2 * hw2;
    float gx = __fadd_rn(up_flow(f, t), rfx_lin(x, W)), gy = __fadd_rn(up_flow(f + hw2, t), rfx_lin(y, H));
    gx = fminf(fmaxf(gx, -1.0f), 1.0f);
    gy = fminf(fmaxf(gy, -1.0f), 1.0f);
    const Corners c = corners(gx, gy, H, W, 0);
    const float* M = k.Hm + i * 9;
    float2 o;
    o.x = 0.f; o.y = 0.f;
    if (c.m_nw) { const float2 v = warp_point(M, c.x0, c.y0, H, W); o.x = fmaf(v.x, c.nw, o.x); o.y = fmaf(v.y, c.nw, o.y); }
    if (c.m_ne) { const float2 v = warp_point(M, c.x0 + 1, c.y0, H, W); o.x = fmaf(v.x, c.ne, o.x); o.y = fmaf(v.y, c.ne, o.y); }
    if (c.m_sw) { const float2 v = warp_point(M, c.x0, c.y0 + 1, H, W); o.x = fmaf(v.x, c.sw, o.x); o.y = fmaf(v.y, c.sw, o.y); }
    if (c.m_se) { const float2 v = warp_point(M, c.x0 + 1, c.y0 + 1, H, W); o.x = fmaf(v.x, c.se, o.x); o.y = fmaf(v.y, c.se, o.y); }
    return o;
}

// flow_i and score_i of homography i at the output pixel (x, y) of a pair, from the record alone.  t = the pixel's /8 taps.
// level 2: flow = compose_flow(flowDown8_i, d2, clamp, inb, flowUp); score = (up(match12) * sample(up(match21), flowUp)) * inb
struct FlowScore { float2 flow; float score; };

__device__ __forceinline__ FlowScore kitti_flow_score(const KittiPair& k, const int i, const int x, const int y, const UpTap& t,
                                                      const bool want_score) {
    const int hw = k.hd * k.wd, H = k.H, W = k.W;
    const float* f = k.flowDown + (size_t)i * 2 * hw;
    float gx = __fadd_rn(up_flow(f, t), rfx_lin(x, W)), gy = __fadd_rn(up_flow(f + hw, t), rfx_lin(y, H));
    gx = fminf(fmaxf(gx, -1.0f), 1.0f);
    gy = fminf(fmaxf(gy, -1.0f), 1.0f);
    const Corners c = corners(gx, gy, H, W, 0);
    float ox = 0.f, oy = 0.f;
    if (c.m_nw) { const float2 v = kitti_d2_point(k, i, c.x0, c.y0); ox = fmaf(v.x, c.nw, ox); oy = fmaf(v.y, c.nw, oy); }
    if (c.m_ne) { const float2 v = kitti_d2_point(k, i, c.x0 + 1, c.y0); ox = fmaf(v.x, c.ne, ox); oy = fmaf(v.y, c.ne, oy); }
    if (c.m_sw) { const float2 v = kitti_d2_point(k, i, c.x0, c.y0 + 1); ox = fmaf(v.x, c.sw, ox); oy = fmaf(v.y, c.sw, oy); }
    if (c.m_se) { const float2 v = kitti_d2_point(k, i, c.x0 + 1, c.y0 + 1); ox = fmaf(v.x, c.se, ox); oy = fmaf(v.y, c.se, oy); }
    FlowScore r;
    r.flow.x = ox; r.flow.y = oy;
    r.score = 0.0f;
    if (want_score) {
        const float inb = (ox >= -1.0f && ox <= 1.0f && oy >= -1.0f && oy <= 1.0f) ? 1.0f : 0.0f;
        const float* m12 = k.matchDown + (size_t)i * 2 * hw;
        const float* s21 = m12 + hw;
        const float v12 = up_resize(m12, t);
        float cyc = 0.0f;
        if (c.m_nw) cyc = fmaf(up_resize(s21, up_tap(k.sh8, k.sw8, c.y0, c.x0, k.hd, k.wd)), c.nw, cyc);
        if (c.m_ne) cyc = fmaf(up_resize(s21, up_tap(k.sh8, k.sw8, c.y0, c.x0 + 1, k.hd, k.wd)), c.ne, cyc);
        if (c.m_sw) cyc = fmaf(up_resize(s21, up_tap(k.sh8, k.sw8, c.y0 + 1, c.x0, k.hd, k.wd)), c.sw, cyc);
        if (c.m_se) cyc = fmaf(up_resize(s21, up_tap(k.sh8, k.sw8, c.y0 + 1, c.x0 + 1, k.hd, k.wd)), c.se, cyc);
        r.score = __fmul_rn(__fmul_rn(v12, cyc), inb);         // (match12 * cycle) * in-bounds, left to right
    }
    return r;
}

// Kernel A.  blockIdx.y = the pair, blockIdx.x strides over its pixels.  scores == NULL (cc_th == 0): the fused walk of
// assemble_records_kernel.  scores != NULL: the owner is found on the pair's FILTERED scores (kitti_scores_records_kernel, then the
// component filter in place), and only the owner's flow is evaluated.
__global__ __launch_bounds__(256) void assemble_kitti_records_kernel(KittiRecArgs a) {
    const KittiPair k = kitti_pair(a, blockIdx.y, a.scores != nullptr);
    if (!k.ok) return;
    const int W = k.W, HW = k.HW, last = k.last;
    float2* __restrict__ flowG = reinterpret_cast<float2*>(a.flowG) + k.out_off;
    float* __restrict__ matchG = a.matchG + k.out_off;
    uint8_t* __restrict__ binary = a.binary + k.out_off;
    const float* __restrict__ sc = a.scores ? a.scores + k.score_off : nullptr;
    const float th = a.th;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += (long long)gridDim.x * blockDim.x) {
        const int p = (int)q;
        const int y = p / W, x = p - y * W;
        const UpTap t = up_tap(k.sh8, k.sw8, y, x, k.hd, k.wd);
        float2 fbest;
        fbest.x = 0.0f; fbest.y = 0.0f;
        float mbest = 0.0f;
        bool found = false;
        if (sc) {
            int best = 0;
            for (int i = 0; i < last; ++i) {
                const float v = sc[(size_t)i * HW + p];
                if (i == 0) mbest = v;
                if (v >= th) {
                    best = i; mbest = v;
                    found = true;
                    break;
                }
            }
            if (last > 0) fbest = kitti_flow_score(k, best, x, y, t, false).flow;
        } else {
            for (int i = 0; i < last; ++i) {
                const FlowScore r = kitti_flow_score(k, i, x, y, t, true);
                // merge_multi_h_kernel's rule: 0 owns the pixel unless a later homography is the first to reach th
                if (i == 0) { mbest = r.score; fbest = r.flow; }
                if (r.score >= th) {
                    mbest = r.score; fbest = r.flow;
                    found = true;
                    break;
                }
            }
        }
        // torch.clamp: a NaN stays a NaN (merge_multi_h_kernel)
        float2 o;
        o.x = fbest.x < -1.0f ? -1.0f : (fbest.x > 1.0f ? 1.0f : fbest.x);
        o.y = fbest.y < -1.0f ? -1.0f : (fbest.y > 1.0f ? 1.0f : fbest.y);
        flowG[p] = o;
        matchG[p] = mbest;
        binary[p] = found ? 1 : 0;
    }
}

// Kernel B (cc_th > 0).  blockIdx.y = pair * max_h + homography: score_i of every map the merge reads (i < last) into the packed
// score buffer, and the map's row (H, W, max_area) of the component filter's table -- (0, 0, 0), which the filter skips, for every
// other map and for a pair whose table row is refused.
__global__ __launch_bounds__(256) void kitti_scores_records_kernel(KittiRecArgs a) {
    const int b = blockIdx.y / a.max_h, i = blockIdx.y - b * a.max_h;
    const KittiPair k = kitti_pair(a, b, true);
    const bool used = k.ok && i < k.last;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int32_t* d = a.dims + 3 * (long long)blockIdx.y;
        d[0] = used ? k.H : 0; d[1] = used ? k.W : 0; d[2] = used ? k.max_area : 0;
    }
    if (!used) return;
    const int W = k.W, HW = k.HW;
    float* __restrict__ sc = a.scores + k.score_off + (size_t)i * HW;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += (long long)gridDim.x * blockDim.x) {
        const int p = (int)q;
        const int y = p / W, x = p - y * W;
        sc[p] = kitti_flow_score(k, i, x, y, up_tap(k.sh8, k.sw8, y, x, k.hd, k.wd), true).score;
    }
}

}  // namespace

// predFlowCoarse's tail (model/model.py:333-340): flowGrad = || f[:, :, 1:, 1:] - f[:, :, :-1, :-1] ||_2 over the two flow
// channels, (B,1,H-1,W-1); flow = clamp(f.permute(0,2,3,1) + grid, -1, 1), (B,H,W,2).  One thread per pixel does both.
__global__ __launch_bounds__(256) void flow_grad_clamp_kernel(const float* __restrict__ f, const float* __restrict__ grid,
                                                             float* __restrict__ flowGrad, float* __restrict__ flow, int B,
                                                             int H, int W, int grid_batch) {
    const long long HW = (long long)H * W, total = (long long)B * HW;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const long long b = q / HW, p = q - b * HW;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const float fx = f[(b * 2) * HW + p], fy = f[(b * 2 + 1) * HW + p];
        const float2 g = reinterpret_cast<const float2*>(grid)[(grid_batch > 1 ? b : 0) * HW + p];
        float2 o;
        o.x = fminf(fmaxf(fx + g.x, -1.0f), 1.0f);
        o.y = fminf(fmaxf(fy + g.y, -1.0f), 1.0f);
        reinterpret_cast<float2*>(flow)[q] = o;
        if (flowGrad && y + 1 < H && x + 1 < W) {
            const float dx = f[(b * 2) * HW + p + W + 1] - fx, dy = f[(b * 2 + 1) * HW + p + W + 1] - fy;
            flowGrad[b * (long long)(H - 1) * (W - 1) + (long long)y * (W - 1) + x] = sqrtf(dx * dx + dy * dy);
        }
    }
}

extern "C" int rfx_warp_grid_f32(const float* Hm, float* grid, int B, int h, int w, void* stream) {
    if (!Hm || !grid || B <= 0 || h <= 0 || w <= 0) return RFX_E_ARG;
    const long long total = (long long)B * h * w;
    const WarpGridArgs a = {Hm, grid, total, h, w};
    return WarpGrid::launch(warp_grid_kernel, a, (unsigned)grid_for(total, WarpGrid::BLOCK), rfx_stream(stream));
}

extern "C" int rfx_grid_sample_f32(const float* in, const float* grid, float* out, int N, int C, int Hi, int Wi,
                                   int Ho, int Wo, int align_corners, void* stream) {
    if (!in || !grid || !out || N <= 0 || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return RFX_E_ARG;
    const long long NP = (long long)N * Ho * Wo;
    const GridSampleArgs a = {in, grid, out, NP, C, Hi, Wi, Ho, Wo, align_corners};
    return GridSample::launch(grid_sample_kernel, a, (unsigned)grid_for(NP, GridSample::BLOCK), rfx_stream(stream));
}

extern "C" int rfx_compose_flow_f32(const float* flowDown, const float* coarseGrid, float* flow12, float* inb,
                                    float* flowUp, int N, int hd, int wd, int Hc, int Wc, int H, int W, int clamp,
                                    void* stream) {
    if (!flowDown || !coarseGrid || !flow12 || N <= 0 || hd <= 0 || wd <= 0 || Hc <= 0 || Wc <= 0 || H <= 0 || W <= 0)
        return RFX_E_ARG;
    const long long NP = (long long)N * H * W;
    const float sh = (float)hd / (float)H, sw = (float)wd / (float)W;
    const ComposeFlowArgs a = {flowDown, coarseGrid, flow12, inb, flowUp, NP, hd, wd, Hc, Wc, H, W, sh, sw, clamp};
    return ComposeFlow::launch(compose_flow_kernel, a, (unsigned)grid_for(NP, ComposeFlow::BLOCK), rfx_stream(stream));
}

extern "C" int rfx_merge_multi_h_f32(const float* flow, const float* match12, long long match12_stride,
                                     const float* cyc, const float* inb, int n, long long HW, float th, int multiH,
                                     float* flowGlobal, float* matchGlobal, uint8_t* binary, void* stream) {
    if (!flow || !match12 || !flowGlobal || n <= 0 || HW <= 0 || match12_stride < HW) return RFX_E_ARG;
    hipLaunchKernelGGL(merge_multi_h_kernel, dim3(grid_for(HW, 256)), dim3(256), 0, rfx_stream(stream), flow, match12,
                       match12_stride, cyc, inb, n, HW, th, multiH, flowGlobal, matchGlobal, binary);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_match_score_f32(const float* match12, long long match12_stride, const float* cyc, const float* inb,
                                   int n, long long HW, float* score, void* stream) {
    if (!match12 || !score || n <= 0 || HW <= 0 || match12_stride < HW) return RFX_E_ARG;
    const long long total = (long long)n * HW;
    hipLaunchKernelGGL(match_score_kernel, dim3(grid_for(total, 256)), dim3(256), 0, rfx_stream(stream), match12,
                       match12_stride, cyc, inb, HW, total, score);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_cycle_tail_f32(const float* flowDown8, const float* match12Down8, long long match12_stride,
                                  const float* match21Down8, long long match21_stride, const float* coarseGrid, float* flow12,
                                  float* match, int N, int hd, int wd, int Hc, int Wc, int H, int W, void* stream) {
    if (!flowDown8 || !match12Down8 || !match21Down8 || !coarseGrid || !flow12 || !match || N <= 0 || hd <= 0 || wd <= 0 || Hc <= 0 ||
        Wc <= 0 || H <= 0 || W <= 0)
        return RFX_E_ARG;
    const long long hw = (long long)hd * wd;
    // plane offsets inside one image are ints in the kernel; the strides may only matter where there is a second image
    if (hw > 0x7fffffffLL || (long long)H * W > 0x7fffffffLL || (N > 1 && (match12_stride < hw || match21_stride < hw))) return RFX_E_ARG;
    const long long NP = (long long)N * H * W;
    const float sh = (float)hd / (float)H, sw = (float)wd / (float)W;
    const CycleTailArgs a = {flowDown8, match12Down8, match21Down8, coarseGrid, flow12, match, NP, match12_stride, match21_stride,
                             hd, wd, Hc, Wc, H, W, sh, sw};
    return CycleTail::launch(cycle_tail_kernel, a, (unsigned)grid_for(NP, CycleTail::BLOCK), rfx_stream(stream));
}

extern "C" int rfx_assemble_records_f32(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                                        const long long* table, int B, long long max_hw, float th, int multiH, int cycle,
                                        const uint8_t* bg, float* flowGlobal, float* matchGlobal, uint8_t* binary,
                                        long long total_px, void* stream) {
    if (!rec || !table || !flowGlobal || !matchGlobal || !binary || B <= 0 || B > 65535 || width <= 0 || max_h <= 0 || off_H < 1 ||
        off_flow < off_H + 9 * max_h || off_flow > width || rec_elems < (long long)B * width || max_hw <= 0 ||
        max_hw > 0x7fffffffLL || total_px < max_hw || ((uintptr_t)flowGlobal & 7))
        return RFX_E_ARG;
    const AssembleRecArgs a = {rec, table, bg, flowGlobal, matchGlobal, binary, rec_elems, total_px,
                               width, max_h, off_H, off_flow, multiH ? 1 : 0, cycle ? 1 : 0, th};
    hipLaunchKernelGGL(assemble_records_kernel, dim3(grid_for(max_hw, 256), B), dim3(256), 0, rfx_stream(stream), a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

namespace {

// the argument checks both KITTI entry points share, before any HIP call
int kitti_records_check(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow, const long long* table,
                        int B, long long max_hw, long long total_px) {
    if (!rec || !table || B <= 0 || width <= 0 || max_h <= 0 || off_H < 1 || off_flow < (long long)off_H + 9LL * max_h ||
        off_flow > width || rec_elems < (long long)B * width || max_hw <= 0 || total_px < max_hw)
        return RFX_E_ARG;
    if (max_hw > 0x7fffffffLL || total_px > 0x7fffffffLL || (long long)B * max_h > 65535) return RFX_E_LIMIT;
    return RFX_OK;
}

}  // namespace

extern "C" int rfx_kitti_scores_records_f32(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                                            const long long* table, int B, long long max_hw, int multiH, float* scores,
                                            long long score_base, long long score_elems, int32_t* dims, long long total_px,
                                            void* stream) {
    if (!scores || !dims || score_base < 0 || score_elems <= 0) return RFX_E_ARG;
    const int rc = kitti_records_check(rec, rec_elems, width, max_h, off_H, off_flow, table, B, max_hw, total_px);
    if (rc != RFX_OK) return rc;
    if (score_elems > 0x7fffffffLL) return RFX_E_LIMIT;
    const KittiRecArgs a = {rec, table, scores, dims, nullptr, nullptr, nullptr, rec_elems, total_px, score_base, score_elems,
                            width, max_h, off_H, off_flow, multiH ? 1 : 0, 0.0f};
    hipLaunchKernelGGL(kitti_scores_records_kernel, dim3(grid_for(max_hw, 256), B * max_h), dim3(256), 0, rfx_stream(stream), a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_assemble_kitti_records_f32(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                                              const long long* table, int B, long long max_hw, float th, int multiH,
                                              const float* scores, long long score_base, long long score_elems, float* flowGlobal,
                                              float* matchGlobal, uint8_t* binary, long long total_px, void* stream) {
    if (!flowGlobal || !matchGlobal || !binary || ((uintptr_t)flowGlobal & 7) || score_base < 0 || (scores && score_elems <= 0))
        return RFX_E_ARG;
    const int rc = kitti_records_check(rec, rec_elems, width, max_h, off_H, off_flow, table, B, max_hw, total_px);
    if (rc != RFX_OK) return rc;
    if (scores && score_elems > 0x7fffffffLL) return RFX_E_LIMIT;
    const KittiRecArgs a = {rec, table, const_cast<float*>(scores), nullptr, flowGlobal, matchGlobal, binary, rec_elems, total_px,
                            score_base, score_elems, width, max_h, off_H, off_flow, multiH ? 1 : 0, th};
    hipLaunchKernelGGL(assemble_kitti_records_kernel, dim3(grid_for(max_hw, 256), B), dim3(256), 0, rfx_stream(stream), a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_flow_grad_clamp_f32(const float* flowCoarse, const float* grid, float* flowGrad, float* flow, int B, int H,
                                       int W, int grid_batch, void* stream) {
    if (!flowCoarse || !grid || !flow || B <= 0 || H <= 0 || W <= 0 || (grid_batch != 1 && grid_batch != B)) return RFX_E_ARG;
    if (flowGrad && (H < 2 || W < 2)) return RFX_E_ARG;
    const long long total = (long long)B * H * W;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(flow_grad_clamp_kernel, dim3(blocks), dim3(256), 0, rfx_stream(stream), flowCoarse, grid, flowGrad, flow, B,
                       H, W, grid_batch);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
