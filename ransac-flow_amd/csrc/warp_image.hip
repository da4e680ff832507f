// warp_image.hip -- the aligned source image (quick_start/align2images.py:97-98,117: F.grid_sample(IsTensor, flow12), ToPILImage,
// fine_aligned_source.png) and its 50 % overlay with the target (:25-28,112: get_Avg_Image) of a whole batch of pairs of any sizes,
// as uint8 HWC images, without a float intermediate.
// (a) rfx_warp_records_u8: from the drivers' device records.  blockIdx.y = the pair, blockIdx.x strides over the pair's own H x W
//     pixels (assemble_records_kernel's mapping and grid cap); a thread evaluates the assembled flow at its pixel from the record alone
//     (assemble_pixel.h) and samples the uint8 source where it lies -- the (B,4) image table carries each pair's source address and
//     size, so sources of any sizes are never concatenated or converted.
// (b) rfx_warp_flow_u8: the same tail on a stored packed flow (the KITTI assembly's, quick-start's flow12, any flow a caller holds).
// Per pixel and channel: ToTensor's x / 255 of each in-image corner (u8_to_f32_kernel, preproc.hip), the bilinear sum in the order
// nw, ne, sw, se with one fused step per corner (grid_sample_body as warp.hip compiles it), clamp to [0, 1], times 255 rounded to
// float32, truncated (ToPILImage's mul(255).byte()).  Output pixels are 3 bytes at arbitrary packed offsets: each thread stores its
// own 3 (+ 3 + 1) bytes, no LDS, no atomics, no workgroup waits on another.
// Built with -ffp-contract=off: every float32 step below is spelled out and rounded as written.
#include "common.h"
#include "assemble_pixel.h"
#include "points_tile.h"

// this unit's own rule from here on, whatever the header above set or the command line says: the only fused steps of the image tail
// are the fmaf calls written below
#pragma clang fp contract(off)

namespace {

constexpr int IMG_COLS = 4;      // image table row: source address | Hs | Ws | target address or 0
constexpr int WARP_BLOCK = 256;

inline int warp_grid_for(long long total) {      // assemble_records_kernel's launch: capped, the kernel strides
    const long long g = (total + WARP_BLOCK - 1) / WARP_BLOCK, cap = 256LL * 32;
    return (int)(g < cap ? g : cap);
}

// Row b of the image table, checked: ok == false for a row without a source or with a size whose pixel count leaves int32.
struct ImagePair { const uint8_t* src; const uint8_t* tgt; int Hs, Ws; bool ok; };

__device__ __forceinline__ ImagePair image_pair(const long long* __restrict__ itable, int b) {
    const long long* __restrict__ T = itable + (long long)b * IMG_COLS;
    const long long src = T[0], Hs = T[1], Ws = T[2], tgt = T[3];
    ImagePair s;
    s.ok = src != 0 && Hs > 0 && Ws > 0 && Hs <= 0x7fffffffLL && Ws <= 0x7fffffffLL && Hs * Ws <= 0x7fffffffLL;
    s.src = reinterpret_cast<const uint8_t*>(src);
    s.tgt = reinterpret_cast<const uint8_t*>(tgt);
    s.Hs = (int)Hs; s.Ws = (int)Ws;
    return s;
}

// The image tail of one output pixel: the source sampled at the normalised point (fx, fy), the overlay with the target's pixel, the
// mask byte.  img / overlay / mask point at the pixel's own bytes (overlay and mask may be null); tpx at the target's pixel or null.
__device__ __forceinline__ void warp_pixel(const ImagePair& s, const float fx, const float fy, const bool bin,
                                           const uint8_t* __restrict__ tpx, uint8_t* __restrict__ img, uint8_t* __restrict__ overlay,
                                           uint8_t* __restrict__ mask) {
    const Corners c = corners(fx, fy, s.Hs, s.Ws, 0);            // on the SOURCE size; a NaN has no in-image corner: the pixel is 0
    const long long row = 3LL * s.Ws;
    const uint8_t* __restrict__ q = s.src + ((long long)c.y0 * s.Ws + c.x0) * 3;      // followed only under a corner's own mask
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float v = 0.0f;
        if (c.m_nw) v = fmaf(__fdiv_rn((float)q[ch], 255.0f), c.nw, v);
        if (c.m_ne) v = fmaf(__fdiv_rn((float)q[3 + ch], 255.0f), c.ne, v);
        if (c.m_sw) v = fmaf(__fdiv_rn((float)q[row + ch], 255.0f), c.sw, v);
        if (c.m_se) v = fmaf(__fdiv_rn((float)q[row + 3 + ch], 255.0f), c.se, v);
        v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
        const uint8_t o = (uint8_t)(int)__fmul_rn(v, 255.0f);   // rounded to float32, then truncated
        img[ch] = o;
        if (overlay && tpx) overlay[ch] = (uint8_t)(((int)o + (int)tpx[ch]) >> 1);
    }
    if (mask) *mask = bin ? 255 : 0;
}

struct WarpRecArgs {
    const float* rec; const long long* table; const long long* itable; const uint8_t* bg; uint8_t* img; uint8_t* overlay; uint8_t* mask;
    long long rec_elems, total_px;           // floats in rec; pixels in each of the packed outputs (and in bg)
    int width, max_h, off_H, off_flow, multiH, cycle; float th;
};

__global__ __launch_bounds__(WARP_BLOCK) void warp_records_u8_kernel(WarpRecArgs a) {
    // rows blockIdx.y of both tables, checked: a row that does not describe a record inside rec, a map inside the outputs and a source
    // is skipped, nothing of it is read or written
    const RecPair k = rec_pair(a.rec, a.rec_elems, a.table, blockIdx.y, a.width, a.max_h, a.off_H, a.off_flow, a.multiH, a.total_px);
    if (!k.ok) return;
    const ImagePair s = image_pair(a.itable, blockIdx.y);
    if (!s.ok) return;
    const int W = k.W, HW = k.HW;
    const uint8_t* __restrict__ bg = a.bg ? a.bg + k.out_off : nullptr;
    uint8_t* __restrict__ img = a.img + 3 * k.out_off;
    uint8_t* __restrict__ overlay = a.overlay ? a.overlay + 3 * k.out_off : nullptr;
    uint8_t* __restrict__ mask = a.mask ? a.mask + k.out_off : nullptr;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += (long long)gridDim.x * blockDim.x) {
        const int p = (int)q;
        const int y = p / W, x = p - y * W;
        const PixelResult r = assemble_pixel(k, y, x, a.cycle, a.th);
        const bool bin = r.found && (!bg || bg[p] != 0);
        warp_pixel(s, r.flow.x, r.flow.y, bin, s.tgt ? s.tgt + 3LL * p : nullptr, img + 3LL * p, overlay ? overlay + 3LL * p : nullptr,
                   mask ? mask + p : nullptr);
    }
}

struct WarpFlowArgs {
    const float* flow; const long long* table; const long long* itable; const uint8_t* binary; uint8_t* img; uint8_t* overlay;
    uint8_t* mask; long long total_px;
};

__global__ __launch_bounds__(WARP_BLOCK) void warp_flow_u8_kernel(WarpFlowArgs a) {
    // row blockIdx.y of the (B,8) table: only H | W | pixel offset (columns 4..6) are read, checked like rec_pair checks them
    const long long* __restrict__ T = a.table + (long long)blockIdx.y * 8;
    const long long Hl = T[4], Wl = T[5], out_off = T[6];
    if (Hl <= 0 || Wl <= 0 || Hl > 0x7fffffffLL || Wl > 0x7fffffffLL || Hl * Wl > 0x7fffffffLL || out_off < 0 ||
        out_off + Hl * Wl > a.total_px)
        return;
    const ImagePair s = image_pair(a.itable, blockIdx.y);
    if (!s.ok) return;
    const int HW = (int)(Hl * Wl);
    const float2* __restrict__ flow = reinterpret_cast<const float2*>(a.flow) + out_off;
    const uint8_t* __restrict__ binary = a.binary ? a.binary + out_off : nullptr;
    uint8_t* __restrict__ img = a.img + 3 * out_off;
    uint8_t* __restrict__ overlay = a.overlay ? a.overlay + 3 * out_off : nullptr;
    uint8_t* __restrict__ mask = (a.mask && binary) ? a.mask + out_off : nullptr;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += (long long)gridDim.x * blockDim.x) {
        const int p = (int)q;
        const float2 f = flow[p];
        warp_pixel(s, f.x, f.y, binary && binary[p] != 0, s.tgt ? s.tgt + 3LL * p : nullptr, img + 3LL * p,
                   overlay ? overlay + 3LL * p : nullptr, mask ? mask + p : nullptr);
    }
}

}  // namespace

extern "C" int rfx_warp_records_u8(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                                   const long long* table, int B, long long max_hw, float th, int multiH, int cycle, const uint8_t* bg,
                                   const long long* itable, uint8_t* img, uint8_t* overlay, uint8_t* mask, long long total_px,
                                   void* stream) {
    if (!rec || !table || !itable || !img || B <= 0 || width <= 0 || max_h <= 0 || off_H < 1 ||
        off_flow < (long long)off_H + 9LL * max_h || off_flow > width || rec_elems < (long long)B * width || max_hw <= 0 ||
        total_px < max_hw || !points_aligned(table, 8) || !points_aligned(itable, 8))
        return RFX_E_ARG;
    if (B > 65535 || max_hw > 0x7fffffffLL) return RFX_E_LIMIT;
    const WarpRecArgs a = {rec, table, itable, bg, img, overlay, mask, rec_elems, total_px,
                           width, max_h, off_H, off_flow, multiH ? 1 : 0, cycle ? 1 : 0, th};
    hipLaunchKernelGGL(warp_records_u8_kernel, dim3(warp_grid_for(max_hw), B), dim3(WARP_BLOCK), 0, rfx_stream(stream), a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_warp_flow_u8(const float* flow, const long long* table, int B, long long max_hw, const uint8_t* binary,
                                const long long* itable, uint8_t* img, uint8_t* overlay, uint8_t* mask, long long total_px,
                                void* stream) {
    if (!flow || !table || !itable || !img || (mask && !binary) || B <= 0 || max_hw <= 0 || total_px < max_hw ||
        !points_aligned(flow, 8) || !points_aligned(table, 8) || !points_aligned(itable, 8))
        return RFX_E_ARG;
    if (B > 65535 || max_hw > 0x7fffffffLL) return RFX_E_LIMIT;
    const WarpFlowArgs a = {flow, table, itable, binary, img, overlay, mask, total_px};
    hipLaunchKernelGGL(warp_flow_u8_kernel, dim3(warp_grid_for(max_hw), B), dim3(WARP_BLOCK), 0, rfx_stream(stream), a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
