// multih.hip -- the host-side glue of the multi-homography rounds as device kernels
// (evaluation/evalHpatch/evaluation.py:211-243, evaluation/evalKITTI/evaluation.py:270-336, utils/outil.py:120).
//
// One round of the reference's loop costs, per pair, a D2H copy of the h x w matchability map, numpy mask algebra, an
// H2D copy of the mask, a bilinear resize + threshold + boolean indexing of the cached matches
// (evaluation/evalHpatch/coarseAlignFeatMatch.py:156-163) and a torch.randint for the RANSAC index draw.  Here a round is
//   filter   (one workgroup per active pair)  explained-region mask -> feature-resolution keep map sampled ONLY at the
//            cells the cached matches point to -> ordered ballot compaction -> match1 / match2 / count, all on the device
//   draw     Philox4x32-10 index draw keyed by (seed, stream, pair, hypothesis), reduced modulo the DEVICE-side match
//            count: no host sync for nbMatch, no 10 000-50 000 x 4 CPU draw + upload per pair and homography
//   accept   gain = mean(newly explained matchability) -> accept rule -> mask update -> result-record store, with ONE
//            small readback (the accept flags) per round for the host's active list.
// The filter and the three accept steps are device functions (filter_body, accept_*_body) with typed parameters: the kernel for
// same-size batches and the one for mixed-size (ragged) batches both call them and differ only in where a pair's data lies.
#include "common.h"
#include <math.h>

namespace {

// ---- Philox4x32-10 (Salmon et al., SC'11; the generator behind torch's device-side randint) -----------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__global__ __launch_bounds__(256) void draw_samples_kernel(const int32_t* __restrict__ n, int64_t* __restrict__ samples, int N,
                                                           uint32_t seed_lo, uint32_t seed_hi, uint32_t str_lo, uint32_t str_hi,
                                                           const int32_t* __restrict__ ids) {
    const int b = blockIdx.y;
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= N) return;
    const int nb = n[b];
    uint32_t c[4] = {(uint32_t)h, (uint32_t)(ids ? ids[b] : b), str_lo, str_hi};
    philox4x32_10(c, seed_lo, seed_hi);
    int64_t* o = samples + ((size_t)b * N + h) * 4;
    // torch's random_from_to for a range below 2^32: (32 random bits) % range + base
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = nb > 0 ? (int64_t)(c[p] % (uint32_t)nb) : 0;
}

// ---- explained-region mask -> keep map at a feature cell ------------------------------------------------------------------
// fg = ((Mask + (1 - bg)) > 0.5) (evaluation/evalHpatch/evaluation.py:212); MtExtend = 1 - fg, bilinear-resized to the target
// feature map (align_corners=False) and thresholded at 0.5 (evaluation/evalHpatch/coarseAlignFeatMatch.py:158-160).
__device__ __forceinline__ float fg_px(float maskv, const float* __restrict__ bg, size_t o) {
    const float bgv = bg ? bg[o] : 1.0f;
    return __fadd_rn(maskv, __fsub_rn(1.0f, bgv)) > 0.5f ? 1.0f : 0.0f;
}

// HAS_MASK = false: nothing is explained yet (the mask is all zero and is not read)
template <bool HAS_MASK = true>
__device__ __forceinline__ float keep_px(const float* __restrict__ mask, const float* __restrict__ bg, size_t o) {
    return __fsub_rn(1.0f, fg_px(HAS_MASK ? mask[o] : 0.0f, bg, o));
}

__device__ __forceinline__ float src_index_nc(float scale, int dst) {   // ATen upsample_bilinear2d, align_corners=False
    const float s = scale * ((float)dst + 0.5f) - 0.5f;
    return s < 0.f ? 0.f : s;
}

template <bool HAS_MASK = true>
__device__ __forceinline__ bool keep_cell(const float* __restrict__ mask, const float* __restrict__ bg, int h, int w, float sh,
                                          float sw, int r, int c) {
    const float fy = src_index_nc(sh, r), fx = src_index_nc(sw, c);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    const float v00 = keep_px<HAS_MASK>(mask, bg, (size_t)y0 * w + x0), v01 = keep_px<HAS_MASK>(mask, bg, (size_t)y0 * w + x1);
    const float v10 = keep_px<HAS_MASK>(mask, bg, (size_t)y1 * w + x0), v11 = keep_px<HAS_MASK>(mask, bg, (size_t)y1 * w + x1);
    // same operation order as resize_bilinear_kernel (pool.hip), which is pinned against ATen
    const float r0 = fmaf(v01, lx, __fmul_rn(v00, hx));
    const float r1 = fmaf(v11, lx, __fmul_rn(v10, hx));
    return fmaf(r1, ly, __fmul_rn(r0, hy)) > 0.5f;
}

__global__ __launch_bounds__(256) void fill_ones_kernel(float* __restrict__ p, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 1.0f;
}

// Ordered ballot compaction of one pair's cached matches: the body both match-filter kernels run, one 1024-thread workgroup per pair.
// Every pointer is already moved to the pair (mask / bg / idx1 / idx2 / xa / ya / xb / yb to pair b, m1 / m2 / kept to slot k); n_out
// is the whole array, indexed with k.  Holds barriers: every thread of the workgroup calls it, as the LAST statement of its kernel.
__device__ __forceinline__ void filter_body(const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2,
                                            const float* __restrict__ mask, const float* __restrict__ bg,
                                            const float* __restrict__ xa, const float* __restrict__ ya,
                                            const float* __restrict__ xb, const float* __restrict__ yb, float* __restrict__ m1,
                                            float* __restrict__ m2, int32_t* __restrict__ n_out, int32_t* __restrict__ kept, int k,
                                            int n, int cap, int h, int w, int ct, float sh, float sw) {
    const int t = threadIdx.x;
    RfxOrderedCompact oc = rfx_ordered_compact_begin();
    for (int s = 0; s < n; s += 1024) {
        const int i = s + t;
        bool keep = false;
        int64_t a = 0, cell = 0;
        if (i < n) {
            a = idx1[i]; cell = idx2[i];
            const int r = (int)(cell / ct), c = (int)(cell - (int64_t)r * ct);
            keep = keep_cell(mask, bg, h, w, sh, sw, r, c);
        }
        const int pos = oc.place(keep);
        if (keep) {
            const size_t o = (size_t)pos * 3;
            m1[o] = xa[a]; m1[o + 1] = ya[a]; m1[o + 2] = 1.0f;
            m2[o] = xb[cell]; m2[o + 1] = yb[cell]; m2[o + 2] = 1.0f;
            if (kept) kept[pos] = i;
        }
    }
    const int ntot = oc.total();
    for (int i = ntot + t; i < cap; i += 1024) {
        const size_t o = (size_t)i * 3;
        m1[o] = m1[o + 1] = m1[o + 2] = 0.0f;
        m2[o] = m2[o + 1] = m2[o + 2] = 0.0f;
        if (kept) kept[i] = -1;
    }
    if (t == 0) n_out[k] = ntot;
}

// One workgroup per active pair: the cached matches of pair b that fall outside the explained region, in order.
__global__ __launch_bounds__(1024) void filter_matches_kernel(
    const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2, const int32_t* __restrict__ count, int cap,
    const int32_t* __restrict__ active, const float* __restrict__ mask, const float* __restrict__ bg, int h, int w, int rt,
    int ct, float sh, float sw, const float* __restrict__ xa, const float* __restrict__ ya, const float* __restrict__ xb,
    const float* __restrict__ yb, float* __restrict__ m1, float* __restrict__ m2, int32_t* __restrict__ n_out,
    int32_t* __restrict__ kept) {
    const int k = blockIdx.x;
    const int b = active ? active[k] : k;
    const int n = count[b];
    const size_t HW = (size_t)h * w;
    mask += (size_t)b * HW;
    if (bg) bg += (size_t)b * HW;
    idx1 += (size_t)b * cap; idx2 += (size_t)b * cap;
    m1 += (size_t)k * cap * 3; m2 += (size_t)k * cap * 3;
    if (kept) kept += (size_t)k * cap;
    filter_body(idx1, idx2, mask, bg, xa, ya, xb, yb, m1, m2, n_out, kept, k, n, cap, h, w, ct, sh, sw);
}

// The whole keep map of the active pairs: what CoarseAlign.getCoarse of variants A / C multiplies the target features with before
// EVERY mutual matching (quick_start/coarseAlignFeatMatch.py:136-143, evaluation/evalYFCC/coarseAlignFeatMatch.py:158-166) --
// keep[k][cell] = 1 where the bilinear-resized (1 - fg) exceeds 0.5, fg = ((mask + (1 - bg)) > 0.5).
__global__ __launch_bounds__(256) void keep_mask_kernel(const float* __restrict__ mask, const float* __restrict__ bg,
                                                        const int32_t* __restrict__ active, int h, int w, int rt, int ct, float sh,
                                                        float sw, float* __restrict__ keep) {
    const int k = blockIdx.y, b = active ? active[k] : k;
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= rt * ct) return;
    const size_t HW = (size_t)h * w;
    const float* m = mask + (size_t)b * HW;
    const float* g = bg ? bg + (size_t)b * HW : nullptr;
    keep[(size_t)k * rt * ct + cell] = keep_cell(m, g, h, w, sh, sw, cell / ct, cell % ct) ? 1.0f : 0.0f;
}

// ---- accept rule ----------------------------------------------------------------------------------------------------
constexpr int NPART = 64;     // partial sums per pair

// mode 0 (evalHpatch/evaluation.py:225,238-239): stat = match * (1 - fg); mask <- (mask + match * (1 - fg)) >= 1
// mode 1 (evalKITTI/evaluation.py:322,332-333):  stat = (match > 0.9999) * (1 - fg); mask <- (mask + match * (1 - fg)) > 0.9999
// The three accept bodies below are what the dense and the ragged kernel of each step both run; the kernels differ only in where a
// pair's maps lie (the element offsets they pass).  Each holds barriers and some leave early behind one: every thread of the
// workgroup calls the body, as the LAST statement of its kernel.

// Accept statistic: partial blockIdx.x of NPART over pair k's HW pixels.  match_off / mask_off: element offsets of the pair's
// matchability map and of its mask (and background map).
__device__ __forceinline__ void accept_partial_body(const float* __restrict__ match, const float* __restrict__ mask,
                                                    const float* __restrict__ bg, int mode, double* __restrict__ part, int k,
                                                    long long HW, size_t match_off, size_t mask_off) {
    match += match_off; mask += mask_off;
    if (bg) bg += mask_off;
    const long long per = (HW + NPART - 1) / NPART;
    const long long p0 = blockIdx.x * per, p1 = p0 + per < HW ? p0 + per : HW;
    double s = 0.0;
    for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
        const float nf = keep_px(mask, bg, (size_t)p);
        const float m = match[p];
        s += (double)__fmul_rn(mode ? (m > 0.9999f ? 1.0f : 0.0f) : m, nf);
    }
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)k * NPART + blockIdx.x] = red[0];
}

// Accept rule and mask update of pair k (batch row b); offsets as in accept_partial_body.
__device__ __forceinline__ void accept_update_body(const float* __restrict__ match, float* __restrict__ mask,
                                                   const float* __restrict__ bg, int mode, const double* __restrict__ part,
                                                   const int32_t* __restrict__ res, const int32_t* __restrict__ n_match,
                                                   const int32_t* __restrict__ nbH, double th, int32_t* __restrict__ accept,
                                                   float* __restrict__ gain, int k, int b, long long HW, size_t match_off,
                                                   size_t mask_off) {
    __shared__ int s_acc;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int q = 0; q < NPART; ++q) s += part[(size_t)k * NPART + q];     // fixed order: every block gets the same sum
        const float g = (float)(s / (double)HW);
        const bool ok = n_match[k] >= 4 && res[k * 4] == 0 && ((double)g > th || nbH[b] == 0);
        s_acc = ok ? 1 : 0;
        if (blockIdx.x == 0) { accept[k] = ok ? 1 : 0; gain[k] = g; }
    }
    __syncthreads();
    if (!s_acc) return;
    match += match_off; mask += mask_off;
    if (bg) bg += mask_off;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
        const float mk = mask[p];
        const float v = __fadd_rn(mk, __fmul_rn(match[p], __fsub_rn(1.0f, fg_px(mk, bg, (size_t)p))));
        mask[p] = (mode ? v > 0.9999f : v >= 1.0f) ? 1.0f : 0.0f;
    }
}

// Record store of pair k (batch row b): hw8 / hwd2 are the pair's /8 and half-resolution /8 pixel counts, off_* the parts of its
// record row, f8_off / m8_off / d2_off the element offsets of pair k's /8 flow, /8 matchability maps and half-resolution flow.
__device__ __forceinline__ void accept_store_body(const int32_t* __restrict__ accept, int32_t* __restrict__ nbH,
                                                  const float* __restrict__ bestH, const float* __restrict__ flow8,
                                                  const float* __restrict__ m12, const float* __restrict__ m21,
                                                  const float* __restrict__ flowd2, float* __restrict__ rec, long long rec_stride,
                                                  int max_h, int k, int b, int hw8, int hwd2, int off_H, int off_flow, int off_match,
                                                  int off_d2, size_t f8_off, size_t m8_off, size_t d2_off) {
    if (!accept[k]) return;
    const int slot = nbH[b];
    const int t = threadIdx.x;
    if (rec && slot < max_h) {
        float* r = rec + (size_t)b * rec_stride;
        if (t < 9) r[off_H + slot * 9 + t] = bestH[k * 9 + t];
        if (flow8)
            for (int i = t; i < 2 * hw8; i += 1024) r[off_flow + (size_t)slot * 2 * hw8 + i] = flow8[f8_off + i];
        if (m12 && m21)
            for (int i = t; i < hw8; i += 1024) {
                r[off_match + (size_t)slot * 2 * hw8 + i] = m12[m8_off + i];
                r[off_match + (size_t)slot * 2 * hw8 + hw8 + i] = m21[m8_off + i];
            }
        if (flowd2)
            for (int i = t; i < 2 * hwd2; i += 1024) r[off_d2 + (size_t)slot * 2 * hwd2 + i] = flowd2[d2_off + i];
    }
    __syncthreads();
    if (t == 0) {
        nbH[b] = slot + 1;
        // the record's nbH field never exceeds the slots it holds; a pair that accepted more (only the unbounded KITTI loop
        // can) is flagged with status 3, and the device counter nbH[] keeps the true number
        if (rec) {
            rec[(size_t)b * rec_stride] = (float)(slot + 1 < max_h ? slot + 1 : max_h);
            rec[(size_t)b * rec_stride + 1] = slot + 1 > max_h ? 3.0f : 0.0f;
        }
    }
}

__global__ __launch_bounds__(256) void accept_partial_kernel(const float* __restrict__ match, const float* __restrict__ mask,
                                                             const float* __restrict__ bg, const int32_t* __restrict__ active,
                                                             long long HW, int mode, double* __restrict__ part) {
    const int k = blockIdx.y, b = active ? active[k] : k;
    accept_partial_body(match, mask, bg, mode, part, k, HW, (size_t)k * HW, (size_t)b * HW);
}

__global__ __launch_bounds__(256) void accept_update_kernel(const float* __restrict__ match, float* __restrict__ mask,
                                                            const float* __restrict__ bg, const int32_t* __restrict__ active,
                                                            long long HW, int mode, const double* __restrict__ part,
                                                            const int32_t* __restrict__ res, const int32_t* __restrict__ n_match,
                                                            const int32_t* __restrict__ nbH, double th,
                                                            int32_t* __restrict__ accept, float* __restrict__ gain) {
    const int k = blockIdx.y, b = active ? active[k] : k;
    accept_update_body(match, mask, bg, mode, part, res, n_match, nbH, th, accept, gain, k, b, HW, (size_t)k * HW, (size_t)b * HW);
}

// The per-pair result record (what evaluation/evalHpatch/evaluation.py:254-260 saves per pair): slot nbH[b] of
// pair b receives H, flowDown8, (match12Down8 | match21Down8) and -- KITTI -- the half-resolution /8 flow; nbH[b] += 1.
__global__ __launch_bounds__(1024) void accept_store_kernel(const int32_t* __restrict__ active, const int32_t* __restrict__ accept,
                                                            int32_t* __restrict__ nbH, const float* __restrict__ bestH,
                                                            const float* __restrict__ flow8, const float* __restrict__ m12,
                                                            const float* __restrict__ m21, int hw8, const float* __restrict__ flowd2,
                                                            int hwd2, float* __restrict__ rec, long long rec_stride, int max_h,
                                                            int off_H, int off_flow, int off_match, int off_d2) {
    const int k = blockIdx.x, b = active ? active[k] : k;
    accept_store_body(accept, nbH, bestH, flow8, m12, m21, flowd2, rec, rec_stride, max_h, k, b, hw8, hwd2, off_H, off_flow, off_match,
                      off_d2, (size_t)k * 2 * hw8, (size_t)k * hw8, (size_t)k * 2 * hwd2);
}

// ---- ragged batches: the active pairs of one launch differ in size ----------------------------------------------------------------
// Pair b's explained-region mask (and background map) lives at element offset moff[b] of ONE packed float buffer; its geometry is row b
// of a device table geom (batch, RG) int32 = h, w, rt, ct, h8, w8.  Every kernel below sets the per-pair values the dense kernel takes
// as launch arguments and then calls the dense kernel's body function (filter_body, accept_*_body): same ballots, same partition of the
// pair's own HW pixels into NPART partial sums, same order of the double additions.
constexpr int RG = 6;

__global__ __launch_bounds__(1024) void filter_matches_ragged_kernel(
    const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2, const int32_t* __restrict__ count, int cap,
    const int32_t* __restrict__ active, const float* __restrict__ mask, const float* __restrict__ bg,
    const long long* __restrict__ moff, const int32_t* __restrict__ geom, const float* __restrict__ xa,
    const float* __restrict__ ya, const long long* __restrict__ offA, const float* __restrict__ xb, const float* __restrict__ yb,
    const long long* __restrict__ offB, float* __restrict__ m1, float* __restrict__ m2, int32_t* __restrict__ n_out,
    int32_t* __restrict__ kept) {
    const int k = blockIdx.x;
    const int b = active ? active[k] : k;
    const int h = geom[b * RG], w = geom[b * RG + 1], rt = geom[b * RG + 2], ct = geom[b * RG + 3];
    const bool sane = h > 0 && w > 0 && rt > 0 && ct > 0;            // a pair with a broken table row keeps no match
    const int n = sane ? (count[b] < cap ? count[b] : cap) : 0;
    // the dense entry point's host-side (float)h / (float)rt: the double quotient of two 24-bit integers rounds to the same float
    const float sh = (float)((double)h / (double)(sane ? rt : 1)), sw = (float)((double)w / (double)(sane ? ct : 1));
    mask += moff[b];
    if (bg) bg += moff[b];
    xa += offA[b]; ya += offA[b]; xb += offB[b]; yb += offB[b];
    idx1 += (size_t)b * cap; idx2 += (size_t)b * cap;
    m1 += (size_t)k * cap * 3; m2 += (size_t)k * cap * 3;
    if (kept) kept += (size_t)k * cap;
    filter_body(idx1, idx2, mask, bg, xa, ya, xb, yb, m1, m2, n_out, kept, k, n, cap, h, w, ct, sh, sw);
}

// keep_mask_kernel for active pairs of different sizes (the per-round re-matching of variant C,
// evaluation/evalYFCC/coarseAlignFeatMatch.py:158-166): workgroup (x, k) computes cells [256 x, 256 x + 256) of pair b = active[k] with
// the pair's own geometry and scales and writes them into ROW b of keep (ldB floats per row: the maskB layout of
// rfx_mutual_nn_ragged_f32); workgroups past the pair's own cell count leave at once.  One thread per active pair stores rt * ct into
// nB_round[b].  mask == nullptr: nothing explained yet; mask == bg == nullptr: every cell is kept.  A pair with a broken table row, or
// more cells than a row holds, gets no cell and nB_round 0.
__global__ __launch_bounds__(256) void keep_mask_ragged_kernel(const float* __restrict__ mask, const float* __restrict__ bg,
                                                               const long long* __restrict__ moff, const int32_t* __restrict__ geom,
                                                               const int32_t* __restrict__ active, int ldB, float* __restrict__ keep,
                                                               int32_t* __restrict__ nB_round) {
    const int k = blockIdx.y, b = active ? active[k] : k;
    const int h = geom[b * RG], w = geom[b * RG + 1], rt = geom[b * RG + 2], ct = geom[b * RG + 3];
    const bool sane = h > 0 && w > 0 && rt > 0 && ct > 0 && (long long)rt * ct <= (long long)ldB;
    const int cells = sane ? rt * ct : 0;
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (nB_round && cell == 0) nB_round[b] = cells;
    if (cell >= cells) return;
    float* out = keep + (size_t)b * ldB + cell;
    if (!mask && !bg) { *out = 1.0f; return; }
    // the dense entry point's host-side (float)h / (float)rt: the double quotient of two 24-bit integers rounds to the same float
    const float sh = (float)((double)h / (double)rt), sw = (float)((double)w / (double)ct);
    const int r = cell / ct, c = cell % ct;
    const bool kept = mask ? keep_cell<true>(mask + moff[b], bg ? bg + moff[b] : nullptr, h, w, sh, sw, r, c)
                           : keep_cell<false>(nullptr, bg + moff[b], h, w, sh, sw, r, c);
    *out = kept ? 1.0f : 0.0f;
}

// match: packed per ACTIVE pair, pair k of the round at element offset match_off[k]; mask / bg: pair b at moff[b]
__global__ __launch_bounds__(256) void accept_partial_ragged_kernel(const float* __restrict__ match,
                                                                    const long long* __restrict__ match_off,
                                                                    const float* __restrict__ mask, const float* __restrict__ bg,
                                                                    const long long* __restrict__ moff, const int32_t* __restrict__ geom,
                                                                    const int32_t* __restrict__ active, int mode,
                                                                    double* __restrict__ part) {
    const int k = blockIdx.y, b = active ? active[k] : k;
    const long long HW = (long long)geom[b * RG] * geom[b * RG + 1];
    accept_partial_body(match, mask, bg, mode, part, k, HW, (size_t)match_off[k], (size_t)moff[b]);
}

__global__ __launch_bounds__(256) void accept_update_ragged_kernel(const float* __restrict__ match, const long long* __restrict__ match_off,
                                                                   float* __restrict__ mask, const float* __restrict__ bg,
                                                                   const long long* __restrict__ moff, const int32_t* __restrict__ geom,
                                                                   const int32_t* __restrict__ active, int mode,
                                                                   const double* __restrict__ part, const int32_t* __restrict__ res,
                                                                   const int32_t* __restrict__ n_match, const int32_t* __restrict__ nbH,
                                                                   double th, int32_t* __restrict__ accept, float* __restrict__ gain) {
    const int k = blockIdx.y, b = active ? active[k] : k;
    const long long HW = (long long)geom[b * RG] * geom[b * RG + 1];
    accept_update_body(match, mask, bg, mode, part, res, n_match, nbH, th, accept, gain, k, b, HW, (size_t)match_off[k],
                       (size_t)moff[b]);
}

// The record row of pair b is laid out with the pair's OWN h8 * w8 (ops.MultiHRecordsRagged); the /8 maps of the round are packed per
// active pair: flowDown8 of pair k at 2 * off8[k], match12Down8 / match21Down8 at off8[k].  KITTI rounds (flowd2 given): the
// half-resolution /8 flow of pair k, 2 * hd2_b * wd2_b floats (d2dims (batch,2) int32 = hd2, wd2 per pair) at 2 * offd2[k], goes to
// the row's flowD2 part, which starts where the dense row of that pair alone has its off_d2: behind the two /8 parts.
__global__ __launch_bounds__(1024) void accept_store_ragged_kernel(const int32_t* __restrict__ active, const int32_t* __restrict__ accept,
                                                                   int32_t* __restrict__ nbH, const float* __restrict__ bestH,
                                                                   const float* __restrict__ flow8, const float* __restrict__ m12,
                                                                   const float* __restrict__ m21, const long long* __restrict__ off8,
                                                                   const int32_t* __restrict__ geom, const float* __restrict__ flowd2,
                                                                   const long long* __restrict__ offd2,
                                                                   const int32_t* __restrict__ d2dims, float* __restrict__ rec,
                                                                   long long rec_stride, int max_h, int off_H, int off_flow) {
    const int k = blockIdx.x, b = active ? active[k] : k;
    const int hw8 = geom[b * RG + 4] * geom[b * RG + 5], hwd2 = flowd2 ? d2dims[2 * b] * d2dims[2 * b + 1] : 0;
    const int off_match = off_flow + 2 * hw8 * max_h, off_d2 = off_match + 2 * hw8 * max_h;
    // off8 / offd2 may be null where the maps they index are not given
    const size_t o8 = off8 ? (size_t)off8[k] : 0, od2 = flowd2 ? (size_t)offd2[k] : 0;
    accept_store_body(accept, nbH, bestH, flow8, m12, m21, flowd2, rec, rec_stride, max_h, k, b, hw8, hwd2, off_H, off_flow, off_match,
                      off_d2, 2 * o8, o8, 2 * od2);
}

}  // namespace

extern "C" int rfx_draw_samples_i64(const int32_t* n, int64_t* samples, int N, int batch, uint64_t seed, uint64_t stream_id,
                                    const int32_t* pair_ids, void* stream) {
    if (!n || !samples || N <= 0 || batch <= 0) return RFX_E_ARG;
    if (batch > 65535) return RFX_E_LIMIT;
    hipLaunchKernelGGL(draw_samples_kernel, dim3((N + 255) / 256, batch), dim3(256), 0, rfx_stream(stream), n, samples, N,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32), pair_ids);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_filter_matches_f32(const int64_t* idx1, const int64_t* idx2, const int32_t* count, int cap,
                                      const int32_t* active, int n_active, const float* mask, const float* bg, int h, int w,
                                      int rt, int ct, const float* xa, const float* ya, const float* xb, const float* yb,
                                      float* match1, float* match2, int32_t* n_out, int32_t* kept, void* stream) {
    if (!idx1 || !idx2 || !count || !mask || !xa || !ya || !xb || !yb || !match1 || !match2 || !n_out || cap <= 0 ||
        n_active <= 0 || h <= 0 || w <= 0 || rt <= 0 || ct <= 0)
        return RFX_E_ARG;
    const float sh = (float)h / (float)rt, sw = (float)w / (float)ct;      // as rfx_resize_bilinear_f32 (align_corners = 0)
    hipLaunchKernelGGL(filter_matches_kernel, dim3(n_active), dim3(1024), 0, rfx_stream(stream), idx1, idx2, count, cap, active,
                       mask, bg, h, w, rt, ct, sh, sw, xa, ya, xb, yb, match1, match2, n_out, kept);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_keep_mask_f32(const float* mask, const float* bg, const int32_t* active, int n_active, int h, int w, int rt,
                                 int ct, float* keep, void* stream) {
    if (!keep || n_active <= 0 || h <= 0 || w <= 0 || rt <= 0 || ct <= 0) return RFX_E_ARG;
    if (n_active > 65535) return RFX_E_LIMIT;
    if (!mask && !bg) {                      // nothing explained, no background map: every cell is kept
        hipLaunchKernelGGL(fill_ones_kernel, dim3(((size_t)n_active * rt * ct + 255) / 256), dim3(256), 0, rfx_stream(stream), keep,
                           (size_t)n_active * rt * ct);
        RFX_LAUNCH_CHECK();
        return RFX_OK;
    }
    const float sh = (float)h / (float)rt, sw = (float)w / (float)ct;      // as rfx_resize_bilinear_f32 (align_corners = 0)
    if (!mask) return RFX_E_ARG;             // a background map without a mask: the caller passes a zero mask
    hipLaunchKernelGGL(keep_mask_kernel, dim3((rt * ct + 255) / 256, n_active), dim3(256), 0, rfx_stream(stream), mask, bg, active, h,
                       w, rt, ct, sh, sw, keep);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" size_t rfx_multih_accept_ws_bytes(int n_active) { return n_active > 0 ? (size_t)n_active * NPART * sizeof(double) : 0; }

extern "C" int rfx_multih_accept_f32(const float* match, float* mask, const float* bg, const int32_t* active, int n_active, int h,
                                     int w, const int32_t* ransac_result, const int32_t* n_match, int32_t* nbH, double th,
                                     int mode, int32_t* accept, float* gain, void* ws, const float* bestH, const float* flowDown8,
                                     const float* match12Down8, const float* match21Down8, int h8, int w8, const float* flowD2,
                                     int hd2, int wd2, float* rec, long long rec_stride, int max_h, int off_H, int off_flow,
                                     int off_match, int off_d2, void* stream) {
    if (!match || !mask || !ransac_result || !n_match || !nbH || !accept || !gain || !ws || n_active <= 0 || h <= 0 || w <= 0 ||
        (mode != 0 && mode != 1))
        return RFX_E_ARG;
    if (rec && (!bestH || max_h <= 0 || rec_stride <= 0)) return RFX_E_ARG;
    if (n_active > 65535) return RFX_E_LIMIT;
    hipStream_t st = rfx_stream(stream);
    const long long HW = (long long)h * w;
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(accept_partial_kernel, dim3(NPART, n_active), dim3(256), 0, st, match, mask, bg, active, HW, mode, part);
    RFX_LAUNCH_CHECK();
    long long g = (HW + 255) / 256;
    if (g > 256) g = 256;
    hipLaunchKernelGGL(accept_update_kernel, dim3((unsigned)g, n_active), dim3(256), 0, st, match, mask, bg, active, HW, mode, part,
                       ransac_result, n_match, nbH, th, accept, gain);
    RFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(accept_store_kernel, dim3(n_active), dim3(1024), 0, st, active, accept, nbH, bestH, flowDown8, match12Down8,
                       match21Down8, h8 * w8, flowD2, hd2 * wd2, rec, rec_stride, max_h, off_H, off_flow, off_match, off_d2);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_filter_matches_ragged_f32(const int64_t* idx1, const int64_t* idx2, const int32_t* count, int cap,
                                             const int32_t* active, int n_active, const float* mask, const float* bg,
                                             const long long* moff, const int32_t* geom, const float* xa, const float* ya,
                                             const long long* offA, const float* xb, const float* yb, const long long* offB,
                                             float* match1, float* match2, int32_t* n_out, int32_t* kept, void* stream) {
    if (!idx1 || !idx2 || !count || !mask || !moff || !geom || !xa || !ya || !offA || !xb || !yb || !offB || !match1 || !match2 ||
        !n_out || cap <= 0 || n_active <= 0)
        return RFX_E_ARG;
    hipLaunchKernelGGL(filter_matches_ragged_kernel, dim3(n_active), dim3(1024), 0, rfx_stream(stream), idx1, idx2, count, cap, active,
                       mask, bg, moff, geom, xa, ya, offA, xb, yb, offB, match1, match2, n_out, kept);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

// rfx_keep_mask_f32 for active pairs of different sizes, one launch (evaluation/evalYFCC/coarseAlignFeatMatch.py:158-166): mask / bg are
// the packed buffers of the ragged rounds (pair b's h * w floats at moff[b]; geom[b] = h, w, rt, ct, h8, w8); bg may be null (all
// foreground), mask may be null (nothing explained yet), both null = every cell kept.  For b = active[k] (k when active is null) the
// first rt * ct floats of row b of keep (ldB floats per row) receive 0 / 1; the rest of the row and the rows of the other pairs are not
// written.  nB_round (or null) receives rt * ct at the active pairs' positions only: zeroed by the caller, it makes
// rfx_mutual_nn_ragged_f32 skip every other pair.  max_cells: the largest rt * ct among the active pairs (sizes the grid).
extern "C" int rfx_keep_mask_ragged_f32(const float* mask, const float* bg, const long long* moff, const int32_t* geom,
                                        const int32_t* active, int n_active, int ldB, int max_cells, float* keep, int32_t* nB_round,
                                        void* stream) {
    if (!moff || !geom || !keep || n_active <= 0 || ldB <= 0 || max_cells <= 0 || max_cells > ldB) return RFX_E_ARG;
    if (n_active > 65535) return RFX_E_LIMIT;
    hipLaunchKernelGGL(keep_mask_ragged_kernel, dim3((max_cells + 255) / 256, n_active), dim3(256), 0, rfx_stream(stream), mask, bg,
                       moff, geom, active, ldB, keep, nB_round);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" size_t rfx_multih_accept_ragged_ws_bytes(int n_active) { return rfx_multih_accept_ws_bytes(n_active); }

namespace {
int accept_ragged(const float* match, const long long* match_off, float* mask, const float* bg, const long long* moff,
                  const int32_t* geom, const int32_t* active, int n_active, long long max_hw, const int32_t* ransac_result,
                  const int32_t* n_match, int32_t* nbH, double th, int mode, int32_t* accept, float* gain, void* ws, const float* bestH,
                  const float* flowDown8, const float* match12Down8, const float* match21Down8, const long long* off8,
                  const float* flowD2, const long long* offd2, const int32_t* d2dims, float* rec, long long rec_stride, int max_h,
                  int off_H, int off_flow, void* stream) {
    if (!match || !match_off || !mask || !moff || !geom || !ransac_result || !n_match || !nbH || !accept || !gain || !ws ||
        n_active <= 0 || max_hw <= 0 || (mode != 0 && mode != 1))
        return RFX_E_ARG;
    if (rec && (!bestH || max_h <= 0 || rec_stride <= 0)) return RFX_E_ARG;
    if ((flowDown8 || match12Down8 || match21Down8) && !off8) return RFX_E_ARG;
    if (flowD2 && (!offd2 || !d2dims)) return RFX_E_ARG;
    if (n_active > 65535) return RFX_E_LIMIT;
    hipStream_t st = rfx_stream(stream);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(accept_partial_ragged_kernel, dim3(NPART, n_active), dim3(256), 0, st, match, match_off, mask, bg, moff, geom,
                       active, mode, part);
    RFX_LAUNCH_CHECK();
    // the update's grid follows the LARGEST pair (max_hw = its h * w): a smaller pair's surplus workgroups find no pixel and leave
    long long g = (max_hw + 255) / 256;
    if (g > 256) g = 256;
    hipLaunchKernelGGL(accept_update_ragged_kernel, dim3((unsigned)g, n_active), dim3(256), 0, st, match, match_off, mask, bg, moff,
                       geom, active, mode, part, ransac_result, n_match, nbH, th, accept, gain);
    RFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(accept_store_ragged_kernel, dim3(n_active), dim3(1024), 0, st, active, accept, nbH, bestH, flowDown8,
                       match12Down8, match21Down8, off8, geom, flowD2, offd2, d2dims, rec, rec_stride, max_h, off_H, off_flow);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
}  // namespace

extern "C" int rfx_multih_accept_ragged_f32(const float* match, const long long* match_off, float* mask, const float* bg,
                                            const long long* moff, const int32_t* geom, const int32_t* active, int n_active,
                                            long long max_hw, const int32_t* ransac_result, const int32_t* n_match, int32_t* nbH,
                                            double th, int mode, int32_t* accept, float* gain, void* ws, const float* bestH,
                                            const float* flowDown8, const float* match12Down8, const float* match21Down8,
                                            const long long* off8, float* rec, long long rec_stride, int max_h, int off_H,
                                            int off_flow, void* stream) {
    return accept_ragged(match, match_off, mask, bg, moff, geom, active, n_active, max_hw, ransac_result, n_match, nbH, th, mode, accept,
                         gain, ws, bestH, flowDown8, match12Down8, match21Down8, off8, nullptr, nullptr, nullptr, rec, rec_stride, max_h,
                         off_H, off_flow, stream);
}

extern "C" int rfx_multih_accept_ragged_d2_f32(const float* match, const long long* match_off, float* mask, const float* bg,
                                               const long long* moff, const int32_t* geom, const int32_t* active, int n_active,
                                               long long max_hw, const int32_t* ransac_result, const int32_t* n_match, int32_t* nbH,
                                               double th, int mode, int32_t* accept, float* gain, void* ws, const float* bestH,
                                               const float* flowDown8, const float* match12Down8, const float* match21Down8,
                                               const long long* off8, const float* flowD2, const long long* offd2,
                                               const int32_t* d2dims, float* rec, long long rec_stride, int max_h, int off_H,
                                               int off_flow, void* stream) {
    if (!flowD2) return RFX_E_ARG;
    return accept_ragged(match, match_off, mask, bg, moff, geom, active, n_active, max_hw, ransac_result, n_match, nbH, th, mode, accept,
                         gain, ws, bestH, flowDown8, match12Down8, match21Down8, off8, flowD2, offd2, d2dims, rec, rec_stride, max_h,
                         off_H, off_flow, stream);
}
