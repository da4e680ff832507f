// warp_image_staged.hip -- EXPERIMENT, not part of librfx: rfx_warp_records_u8 with the output bytes of a workgroup's 256 pixels
// staged in LDS and written as aligned dwords, to measure against the product's per-thread byte stores (DESIGN "Aligned images of a
// batch from its records"; scripts/ubench/warp_image_bench.py --staged-lib; figures in profiles/warp_image_bench.json under
// "lds_staged").  Everything but the stores is the product's code: this file includes csrc/warp_image.hip (its entry point renamed)
// and uses its argument block, row checks and warp_pixel.  Built as a small library that defines the one entry point and takes
// every other symbol from librfx.so:
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -shared -o ransac-flow_amd/librfx_warp_staged.so \
//           scripts/ubench/warp_image_staged.hip -Lransac-flow_amd -lrfx -Wl,-rpath,'$ORIGIN'
//     python scripts/ubench/warp_image_bench.py --staged-lib ransac-flow_amd/librfx_warp_staged.so
// (RFX_LIB=ransac-flow_amd/librfx_warp_staged.so runs anything else, tests/test_gpu_warp_image.py for one, on this variant.)
// A trip of a workgroup covers 256 consecutive pixels of one pair = up to 768 consecutive output bytes starting at any byte address.
// The bytes are staged at the address's offset inside its dword, so that LDS dword i is global dword i of the aligned span; whole
// dwords go out as dwords, the (at most two) partial ones byte by byte.  The mask is one byte per pixel and stays a byte store.
#define rfx_warp_records_u8 rfx_warp_records_u8_bytes
#include "../../ransac-flow_amd/csrc/warp_image.hip"
#undef rfx_warp_records_u8

namespace {

constexpr int STAGE_WORDS = (3 + 3 * WARP_BLOCK + 3) / 4;      // 193 dwords hold any 768 bytes shifted by up to 3

// bytes [shift, shift + n) of lds -> g[0, n), g = G + shift with G 4-byte aligned
__device__ __forceinline__ void staged_out(uint8_t* __restrict__ g, const uint32_t* __restrict__ ldsw, const int shift, const int n) {
    uint8_t* __restrict__ G = g - shift;
    const uint8_t* __restrict__ lds = reinterpret_cast<const uint8_t*>(ldsw);
    const int i = threadIdx.x, lo = 4 * i, hi = lo + 4;
    if (lo >= shift + n || hi <= shift) return;
    if (lo >= shift && hi <= shift + n) {
        *reinterpret_cast<uint32_t*>(G + lo) = ldsw[i];
    } else {
        for (int j = lo; j < hi; ++j)
            if (j >= shift && j < shift + n) G[j] = lds[j];
    }
}

__global__ __launch_bounds__(WARP_BLOCK) void warp_records_u8_staged_kernel(WarpRecArgs a) {
    __shared__ uint32_t stage[2][STAGE_WORDS];
    const RecPair k = rec_pair(a.rec, a.rec_elems, a.table, blockIdx.y, a.width, a.max_h, a.off_H, a.off_flow, a.multiH, a.total_px);
    if (!k.ok) return;                                         // (the same for every thread of the workgroup)
    const ImagePair s = image_pair(a.itable, blockIdx.y);
    if (!s.ok) return;
    const int W = k.W, HW = k.HW, t = threadIdx.x;
    const uint8_t* __restrict__ bg = a.bg ? a.bg + k.out_off : nullptr;
    uint8_t* __restrict__ img = a.img + 3 * k.out_off;
    const bool with_overlay = a.overlay && s.tgt;
    uint8_t* __restrict__ overlay = with_overlay ? a.overlay + 3 * k.out_off : nullptr;
    uint8_t* __restrict__ mask = a.mask ? a.mask + k.out_off : nullptr;
    uint8_t* limg = reinterpret_cast<uint8_t*>(stage[0]);
    uint8_t* lov = reinterpret_cast<uint8_t*>(stage[1]);
    for (long long base = (long long)blockIdx.x * WARP_BLOCK; base < HW; base += (long long)gridDim.x * WARP_BLOCK) {
        const int cnt = HW - base < WARP_BLOCK ? (int)(HW - base) : WARP_BLOCK;
        uint8_t* gi = img + 3 * base;
        uint8_t* go = with_overlay ? overlay + 3 * base : nullptr;
        const int si = (int)((uintptr_t)gi & 3), so = (int)((uintptr_t)go & 3);
        if (t < cnt) {
            const int p = (int)base + t;
            const int y = p / W, x = p - y * W;
            const PixelResult r = assemble_pixel(k, y, x, a.cycle, a.th);
            const bool bin = r.found && (!bg || bg[p] != 0);
            warp_pixel(s, r.flow.x, r.flow.y, bin, s.tgt ? s.tgt + 3LL * p : nullptr, limg + si + 3 * t, with_overlay ? lov + so + 3 * t : nullptr,
                       mask ? mask + p : nullptr);
        }
        __syncthreads();
        staged_out(gi, stage[0], si, 3 * cnt);
        if (with_overlay) staged_out(go, stage[1], so, 3 * cnt);
        __syncthreads();
    }
}

}  // namespace

extern "C" int rfx_warp_records_u8(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                                   const long long* table, int B, long long max_hw, float th, int multiH, int cycle, const uint8_t* bg,
                                   const long long* itable, uint8_t* img, uint8_t* overlay, uint8_t* mask, long long total_px,
                                   void* stream) {
    if (!rec || !table || !itable || !img || B <= 0 || B > 65535 || width <= 0 || max_h <= 0 || off_H < 1 ||
        off_flow < (long long)off_H + 9LL * max_h || off_flow > width || rec_elems < (long long)B * width || max_hw <= 0 ||
        max_hw > 0x7fffffffLL || total_px < max_hw || !points_aligned(table, 8) || !points_aligned(itable, 8))
        return RFX_E_ARG;
    const WarpRecArgs a = {rec, table, itable, bg, img, overlay, mask, rec_elems, total_px,
                           width, max_h, off_H, off_flow, multiH ? 1 : 0, cycle ? 1 : 0, th};
    hipLaunchKernelGGL(warp_records_u8_staged_kernel, dim3(warp_grid_for(max_hw), B), dim3(WARP_BLOCK), 0, rfx_stream(stream), a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
