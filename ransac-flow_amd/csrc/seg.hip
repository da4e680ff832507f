// seg.hip -- the element-wise / small-reduction kernels of the sky-segmentation forward pass (segNet/segEval.py:23-43
// on top of segNet/segModel.py:218-265): everything of SegNet.getSky that is not a convolution (those run on the convolution
// family: conv.hip incl. the dilated entry point, conv3x3.hip, conv1x1.hip), a bilinear resize (pool.hip) or a max-pool.
//   adaptive_avgpool   nn.AdaptiveAvgPool2d(s), s = 1 / 2 / 3 / 6 on the 2048-channel conv5 map   (segModel.py:227)
//   softmax_accum      scores += softmax(logits, dim=1) / 5 at the original image size             (segModel.py:258, segEval.py:34-35)
//   argmax_mask        torch.max(scores, dim=1) -> (pred == segId) as a float32 mask               (segEval.py:37-43)
//   seg_vote           bilinear up-sampling of the S scales' logits + softmax_accum + argmax_mask per pixel, nothing of size C*H*W written
//   sky_bytes / less_than   the scripts' imresize(mask, (h, w)) < 128 around the two resampler passes (evalYFCC/evaluation.py:193-201)
// HBM-bound, one thread per output element / pixel, fp32, the summation orders of the ATen CPU kernels (row-major window
// sum; max-subtracted softmax with one pass for the sum).
#include "group.h"
#include <math.h>

namespace {

inline int grid_for(long long total, int block) {
    long long g = (total + block - 1) / block;
    const long long cap = 256LL * 32;
    return (int)(g < cap ? g : cap);
}

// ATen adaptive_avg_pool2d (CPU): window [floor(o*In/Out), ceil((o+1)*In/Out)), values summed row-major, divided by the count
__global__ __launch_bounds__(256) void adaptive_avgpool_kernel(const float* __restrict__ in, float* __restrict__ out, long long total,
                                                               int Hin, int Win, int Hout, int Wout) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int ow = (int)(idx % Wout);
        const long long r = idx / Wout;
        const int oh = (int)(r % Hout);
        const long long nc = r / Hout;
        const int h0 = (oh * Hin) / Hout, h1 = ((oh + 1) * Hin + Hout - 1) / Hout;
        const int w0 = (ow * Win) / Wout, w1 = ((ow + 1) * Win + Wout - 1) / Wout;
        const float* src = in + nc * Hin * Win;
        float s = 0.0f;
        for (int h = h0; h < h1; ++h)
            for (int w = w0; w < w1; ++w) s += src[(size_t)h * Win + w];
        out[idx] = s / (float)((h1 - h0) * (w1 - w0));
    }
}

// scores[n, c, p] (+)= softmax_c(logits[n, :, p]) / div      (C channel planes of HW pixels each)
__global__ __launch_bounds__(256) void softmax_accum_kernel(const float* __restrict__ logits, float* __restrict__ scores, long long NP,
                                                            int C, long long HW, float div, int accumulate) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < NP; idx += (long long)gridDim.x * blockDim.x) {
        const long long n = idx / HW, p = idx - n * HW;
        const float* src = logits + (size_t)n * C * HW + p;
        float* dst = scores + (size_t)n * C * HW + p;
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) { const float v = src[(size_t)c * HW]; mx = v > mx ? v : mx; }
        float sum = 0.0f;
        for (int c = 0; c < C; ++c) sum += expf(src[(size_t)c * HW] - mx);
        for (int c = 0; c < C; ++c) {
            const float pr = expf(src[(size_t)c * HW] - mx) / sum / div;
            dst[(size_t)c * HW] = accumulate ? dst[(size_t)c * HW] + pr : pr;
        }
    }
}

// pred = first arg-max over the C planes; mask = (pred == id) or its complement, float32; pred_out optional (int32)
__global__ __launch_bounds__(256) void argmax_mask_kernel(const float* __restrict__ scores, long long NP, int C, long long HW, int id,
                                                          int complement, float* __restrict__ mask, int32_t* __restrict__ pred_out) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < NP; idx += (long long)gridDim.x * blockDim.x) {
        const long long n = idx / HW, p = idx - n * HW;
        const float* src = scores + (size_t)n * C * HW + p;
        float best = src[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = src[(size_t)c * HW];
            if (v > best || (v != v && best == best)) { best = v; arg = c; }     // strict >: the first maximum; NaN wins like torch.max
        }
        const float hit = arg == id ? 1.0f : 0.0f;
        mask[idx] = complement ? 1.0f - hit : hit;
        if (pred_out) pred_out[idx] = arg;
    }
}

}  // namespace

extern "C" int rfx_adaptive_avgpool2d_f32(const float* in, float* out, int NC, int Hin, int Win, int Hout, int Wout, void* stream) {
    if (!in || !out || NC <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return RFX_E_ARG;
    const long long total = (long long)NC * Hout * Wout;
    hipLaunchKernelGGL(adaptive_avgpool_kernel, dim3(grid_for(total, 256)), dim3(256), 0, rfx_stream(stream), in, out, total, Hin, Win,
                       Hout, Wout);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_softmax_accum_f32(const float* logits, float* scores, int N, int C, long long HW, float div, int accumulate,
                                     void* stream) {
    if (!logits || !scores || N <= 0 || C <= 0 || HW <= 0 || !(div > 0.0f)) return RFX_E_ARG;
    const long long NP = (long long)N * HW;
    hipLaunchKernelGGL(softmax_accum_kernel, dim3(grid_for(NP, 256)), dim3(256), 0, rfx_stream(stream), logits, scores, NP, C, HW, div,
                       accumulate);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_argmax_mask_f32(const float* scores, int N, int C, long long HW, int id, int complement, float* mask,
                                   int32_t* pred, void* stream) {
    if (!scores || !mask || N <= 0 || C <= 0 || HW <= 0) return RFX_E_ARG;
    const long long NP = (long long)N * HW;
    hipLaunchKernelGGL(argmax_mask_kernel, dim3(grid_for(NP, 256)), dim3(256), 0, rfx_stream(stream), scores, NP, C, HW, id, complement,
                       mask, pred);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// seg_vote: what rfx_resize_bilinear_f32(align_corners = 0) -> rfx_softmax_accum_f32 per scale -> rfx_argmax_mask_f32 give, per pixel,
// without the (N, C, H, W) up-sampled logits and scores in between.  The logit maps of the S scales are a few MB and stay in cache;
// the four-tap value is recomputed in each of the three class loops.
namespace {

constexpr int SEG_VOTE_MAX_SCALES = 8;

struct SegVoteArgs {
    const float* src[SEG_VOTE_MAX_SCALES];   // (N, C, h[s], w[s])
    int h[SEG_VOTE_MAX_SCALES], w[SEG_VOTE_MAX_SCALES];
    float sh[SEG_VOTE_MAX_SCALES], sw[SEG_VOTE_MAX_SCALES];   // (float)h / (float)H, (float)w / (float)W: rfx_resize_bilinear_f32's
    int S, C, H, W;
    long long NP;                            // N * H * W
    float div;
    int id, complement;
    float* mask;
    int32_t* pred;
};

// ATen upsample_bilinear2d index rule for align_corners = false (pool.hip's src_index)
__device__ __forceinline__ float vote_src_index(float scale, int dst) {
    const float s = scale * ((float)dst + 0.5f) - 0.5f;
    return s < 0.f ? 0.f : s;
}

// the taps of one scale at one output pixel: the upper left tap's offset inside a plane, the steps to the clamped right and lower
// neighbours (dx = 0 / 1, dy = 0 / the row pitch) and resize_bilinear_body's two fractions
struct VoteTap { int o00, dx, dy; float lx, ly; };

// resize_bilinear_body's per-sample expression, operation for operation: __fmul_rn, then fmaf
__device__ __forceinline__ float vote_sample(const float* __restrict__ plane, const VoteTap& t) {
    const float* q = plane + t.o00;
    const float v00 = q[0], v01 = q[t.dx], v10 = q[t.dy], v11 = q[t.dy + t.dx];
    const float hy = 1.f - t.ly, hx = 1.f - t.lx;
    const float r0 = fmaf(v01, t.lx, __fmul_rn(v00, hx));
    const float r1 = fmaf(v11, t.lx, __fmul_rn(v10, hx));
    return fmaf(r1, t.ly, __fmul_rn(r0, hy));
}

__device__ __forceinline__ void seg_vote_body(const SegVoteArgs& a, const unsigned bx, const unsigned gx) {
    constexpr int MS = SEG_VOTE_MAX_SCALES;
    const int S = a.S, C = a.C, H = a.H, W = a.W;
    const long long HW = (long long)H * W;
    for (long long idx = (long long)bx * blockDim.x + threadIdx.x; idx < a.NP; idx += (long long)gx * blockDim.x) {
        const long long n = idx / HW;
        const int p = (int)(idx - n * HW);
        const int oy = p / W, ox = p - oy * W;
        VoteTap tap[MS];
        const float* base[MS];
        int plane[MS];                           // h * w <= 2^31 - 1 (checked by the entry point)
        float mx[MS], sum[MS];
#pragma unroll
        for (int s = 0; s < MS; ++s) {
            if (s < S) {
                const int Hin = a.h[s], Win = a.w[s];
                const float fy = vote_src_index(a.sh[s], oy), fx = vote_src_index(a.sw[s], ox);
                int y0 = (int)fy, x0 = (int)fx;
                y0 = y0 < Hin - 1 ? y0 : Hin - 1;      // (never taken by an index the rule above produces: keeps every read inside the plane)
                x0 = x0 < Win - 1 ? x0 : Win - 1;
                tap[s].ly = fy - (float)y0;
                tap[s].lx = fx - (float)x0;
                tap[s].o00 = y0 * Win + x0;
                tap[s].dx = x0 < Win - 1 ? 1 : 0;
                tap[s].dy = y0 < Hin - 1 ? Win : 0;
                plane[s] = Hin * Win;
                base[s] = a.src[s] + (size_t)n * C * plane[s];
                mx[s] = -INFINITY;
                sum[s] = 0.0f;
            }
        }
        // softmax_accum_kernel's three loops, per scale: the maximum, the sum of expf(v - mx) in class order, the probabilities
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int s = 0; s < MS; ++s)
                if (s < S) { const float v = vote_sample(base[s] + (size_t)c * plane[s], tap[s]); mx[s] = v > mx[s] ? v : mx[s]; }
        }
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int s = 0; s < MS; ++s)
                if (s < S) sum[s] += expf(vote_sample(base[s] + (size_t)c * plane[s], tap[s]) - mx[s]);
        }
        float best = 0.0f;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            // the first scale stores p_0, every other one adds its own: ((p_0 + p_1) + ...)
            float score = expf(vote_sample(base[0] + (size_t)c * plane[0], tap[0]) - mx[0]) / sum[0] / a.div;
#pragma unroll
            for (int s = 1; s < MS; ++s)
                if (s < S) score = score + expf(vote_sample(base[s] + (size_t)c * plane[s], tap[s]) - mx[s]) / sum[s] / a.div;
            // argmax_mask_kernel: strict >, the first maximum; NaN wins like torch.max
            if (c == 0 || score > best || (score != score && best == best)) { best = score; arg = c; }
        }
        const float hit = arg == a.id ? 1.0f : 0.0f;
        a.mask[idx] = a.complement ? 1.0f - hit : hit;
        if (a.pred) a.pred[idx] = arg;
    }
}

using SegVote = RfxFamily<SegVoteArgs, seg_vote_body, 256>;
__global__ __launch_bounds__(SegVote::BLOCK) void seg_vote_kernel(SegVoteArgs a) { seg_vote_body(a, blockIdx.x, gridDim.x); }

// bit 0: the map holds a zero, bit 1: it holds a non-zero value.  Only ORs of constants reach the word, so it does not depend on the
// order in which workgroups run.  A wavefront whose pixels lie in one map sends one atomic for all its lanes.
__global__ __launch_bounds__(256) void sky_flags_kernel(const float* __restrict__ mask, long long NP, long long HW, int32_t* __restrict__ flags) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < NP; idx += (long long)gridDim.x * blockDim.x) {
        const bool nz = mask[idx] != 0.0f;
        const int n = (int)(idx / HW);
        const unsigned long long act = __ballot(1), bnz = __ballot(nz);
        const int first = __ffsll((long long)act) - 1;
        if (__all(n == __shfl(n, first))) {
            if ((int)(threadIdx.x & 63) == first) atomicOr(&flags[n], (bnz ? 2 : 0) | ((act & ~bnz) ? 1 : 0));
        } else {
            atomicOr(&flags[n], nz ? 2 : 1);
        }
    }
}

// bytescale of a 0/1 map (scipy 1.2.3 pilutil.bytescale: cscale = (cmax - cmin) or 1 -> a constant map becomes zeros) and
// np.rot90(bytes, k): out (N, Ho, Wo) with (Ho, Wo) = (H, W) for even k, (W, H) for odd k
__global__ __launch_bounds__(256) void sky_bytes_kernel(const float* __restrict__ mask, const int32_t* __restrict__ flags, long long NP,
                                                        int H, int W, int k, uint8_t* __restrict__ out) {
    const int Wo = (k & 1) ? H : W;
    const long long HW = (long long)H * W;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < NP; idx += (long long)gridDim.x * blockDim.x) {
        const long long n = idx / HW;
        const int p = (int)(idx - n * HW);
        const int i = p / Wo, j = p - i * Wo;
        int r, c;                                     // np.rot90(m, k)[i, j] = m[r, c]
        if (k == 0) { r = i; c = j; }
        else if (k == 1) { r = j; c = W - 1 - i; }
        else if (k == 2) { r = H - 1 - i; c = W - 1 - j; }
        else { r = H - 1 - j; c = i; }
        const float v = mask[n * HW + (long long)r * W + c];
        out[idx] = (flags[n] == 3 && v != 0.0f) ? 255 : 0;
    }
}

__global__ __launch_bounds__(256) void less_than_u8_kernel(const uint8_t* __restrict__ in, long long total, int thr, float* __restrict__ out) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x)
        out[idx] = (int)in[idx] < thr ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int rfx_seg_vote_f32(const float* const* logits, const int32_t* hs, const int32_t* ws, int S, int N, int C, int H, int W,
                                float div, int id, int complement, float* mask, int32_t* pred, void* stream) {
    if (!logits || !hs || !ws || !mask || S < 1 || S > SEG_VOTE_MAX_SCALES || N <= 0 || C <= 0 || H <= 0 || W <= 0 || !(div > 0.0f))
        return RFX_E_ARG;
    SegVoteArgs a = {};
    for (int s = 0; s < S; ++s) {
        if (!logits[s] || hs[s] <= 0 || ws[s] <= 0) return RFX_E_ARG;
        if ((long long)hs[s] * ws[s] > 0x7fffffffLL) return RFX_E_LIMIT;      // tap offsets inside a plane are int32
        a.src[s] = logits[s];
        a.h[s] = hs[s];
        a.w[s] = ws[s];
        a.sh[s] = (float)hs[s] / (float)H;
        a.sw[s] = (float)ws[s] / (float)W;
    }
    const long long NP = (long long)N * H * W;
    if (NP > 0x7fffffffLL) return RFX_E_LIMIT;
    a.S = S; a.C = C; a.H = H; a.W = W; a.NP = NP; a.div = div; a.id = id; a.complement = complement; a.mask = mask; a.pred = pred;
    return SegVote::launch(seg_vote_kernel, a, (unsigned)grid_for(NP, SegVote::BLOCK), rfx_stream(stream));
}

extern "C" size_t rfx_sky_bytes_ws_bytes(int N) { return N > 0 ? (size_t)N * sizeof(int32_t) : 0; }

extern "C" int rfx_sky_bytes_u8(const float* mask, int N, int H, int W, int k, uint8_t* out, void* ws, void* stream) {
    if (!mask || !out || !ws || N <= 0 || H <= 0 || W <= 0 || k < 0 || k > 3) return RFX_E_ARG;
    const long long HW = (long long)H * W, NP = (long long)N * HW;
    if (NP > 0x7fffffffLL) return RFX_E_LIMIT;
    int32_t* flags = static_cast<int32_t*>(ws);
    hipError_t e = hipMemsetAsync(flags, 0, (size_t)N * sizeof(int32_t), rfx_stream(stream));
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sky_flags_kernel, dim3(grid_for(NP, 256)), dim3(256), 0, rfx_stream(stream), mask, NP, HW, flags);
    RFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sky_bytes_kernel, dim3(grid_for(NP, 256)), dim3(256), 0, rfx_stream(stream), mask, flags, NP, H, W, k, out);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_less_than_u8_f32(const uint8_t* in, long long total, int threshold, float* out, void* stream) {
    if (!in || !out || total <= 0) return RFX_E_ARG;
    hipLaunchKernelGGL(less_than_u8_kernel, dim3(grid_for(total, 256)), dim3(256), 0, rfx_stream(stream), in, total, threshold, out);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
