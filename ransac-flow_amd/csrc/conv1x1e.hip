// conv1x1e.hip -- the 64 -> 256 expansions of the trunk's layer1 (Bottleneck conv3 and the projection shortcut,
// model/resnet50.py:77-79,139-143) on the fp32 MFMA: a 1x1 / stride 1 convolution that KNOWS K = 64.
//
// conv1x1.hip's k-major kernel runs these layers as 128-channel x 128-pixel tiles with two K steps: two workgroups per pixel tile
// each stage the same 32 KB input panel and 32 KB of weights, and the cross-tile pipeline is mostly prologue and epilogue.  The
// layers are bound by the bytes a CU moves, not by its matrix pipe, so here
//   * the whole wT[64][256] matrix (64 KB) is copied into LDS ONCE per persistent workgroup (one per CU);
//   * a WAVEFRONT owns a 32-pixel tile and produces ALL output channels of it: its B operands -- lane (k & 1 = lane >> 5,
//     p = lane & 31) of k pair kk holds in[2 kk + (lane >> 5)][p] -- are 32 coalesced dword loads straight into registers, read
//     from memory exactly once and never staged; the A operand of an MFMA is one ds_read_b32 at an immediate offset of the
//     resident weights (32 consecutive lanes read 32 consecutive floats: no bank conflict);
//   * there is no barrier after the weight copy: the 8 wavefronts of a workgroup (2 per SIMD) walk their tiles independently,
//     so one wavefront's epilogue (residual loads, stores) runs under the other's MFMAs.
// Two-source form: out = relu(fmaf(acc_a, scale_a, shift_a) + d), d = fmaf(acc_b, scale_b, shift_b) from a second input / weight
// set over the same pixels -- Bottleneck block 0, whose projected shortcut d then never goes to memory.  Per channel pass the
// shortcut GEMM runs first, d is finalised in registers (rounded to float32), then the main GEMM accumulates and the shared
// epilogue (conv_epilogue.h, its PRE form) adds d: the operations of the two launches it replaces, in their order.
// k runs in the same pairs and the same ascending order as in conv1x1.hip, one chain per output: bit-identical results.
#include "common.h"
#include "conv_epilogue.h"
#include "group.h"
#include <type_traits>

namespace {

constexpr int E64_K = 64;          // input channels
constexpr int E64_MAXC = 256;      // output channels the resident weights are sized for (row stride of the LDS image)
constexpr int E64_WAVES = 8;       // wavefronts per workgroup
constexpr int E64_PIX = 32;        // pixels per wavefront tile
// 32-channel sub-tiles per channel pass.  Plain form: 128 channels (244 registers).  Two-source form: 64 channels -- d and the
// accumulators of a 128-channel pass beside both operand sets spill (103 registers); with 64 it holds 256 and no scratch.
constexpr int E64_PLAIN_NS = 4, E64_DUAL_NS = 2;

struct E64Args {
    const float* in[2]; const float* wT[2]; const float* scale[2]; const float* shift[2];   // [0]: main GEMM, [1]: shortcut (two-source)
    const float* res; float* out;
    int HW, Cout, act;
    long long P;       // N*HW
    long long tiles;   // 32-pixel tiles
};

template <bool TWO, int NS>
__global__ __launch_bounds__(E64_WAVES * 64) void conv1x1_expand64_kernel(E64Args a) {
    constexpr int SRC = TWO ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float Ws[SRC][E64_K][E64_MAXC];
    __shared__ float s_scale[SRC][E64_MAXC], s_shift[SRC][E64_MAXC];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lrow = lane >> 5, lcol = lane & 31;
    const size_t HW = (size_t)a.HW;

    // resident operands: wT[k][Mpad = Cout] -> Ws[k][E64_MAXC], the folded BatchNorm vectors
    const int c4 = a.Cout / 4;
#pragma unroll
    for (int s = 0; s < SRC; ++s) {
        for (int i = t; i < E64_K * c4; i += E64_WAVES * 64) {
            const int k = i / c4, c = i - k * c4;
            *reinterpret_cast<f32x4*>(&Ws[s][k][c * 4]) = *reinterpret_cast<const f32x4*>(a.wT[s] + (size_t)k * a.Cout + c * 4);
        }
        if (t < a.Cout) {
            s_scale[s][t] = a.scale[s] ? a.scale[s][t] : 1.0f;
            s_shift[s][t] = a.shift[s] ? a.shift[s][t] : 0.0f;
        }
    }
    __syncthreads();

    const long long stride = (long long)gridDim.x * E64_WAVES;
    for (long long tile = (long long)blockIdx.x * E64_WAVES + wave; tile < a.tiles; tile += stride) {
        // this lane's pixel (columns past the last pixel compute on a valid address and store nothing)
        long long pp = tile * E64_PIX + lcol;
        bool pix_ok[1] = {pp < a.P};
        if (!pix_ok[0]) pp = a.P - 1;
        const long long n = pp / a.HW;
        const size_t hw = (size_t)(pp - n * a.HW);
        const size_t in_off = ((size_t)n * E64_K + lrow) * HW + hw;
        size_t pix_off[1] = {(size_t)n * a.Cout * HW + hw};

        float xv[SRC][E64_K / 2];
#pragma unroll
        for (int s = SRC - 1; s >= 0; --s)       // the shortcut's operands first: its GEMM runs first
#pragma unroll
            for (int kk = 0; kk < E64_K / 2; ++kk) xv[s][kk] = a.in[s][in_off + (size_t)(2 * kk) * HW];

        for (int m0 = 0; m0 < a.Cout; m0 += 32 * NS) {
            auto gemm = [&](auto src, f32x16 (&acc)[NS][1]) {
                constexpr int s = decltype(src)::value;      // compile-time: xv stays in registers
                const float* wp = &Ws[s][lrow][m0 + lcol];
#pragma unroll
                for (int i = 0; i < NS; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.0f;
#pragma unroll
                for (int kk = 0; kk < E64_K / 2; ++kk)
#pragma unroll
                    for (int i = 0; i < NS; ++i)
                        acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[2 * kk * E64_MAXC + i * 32], xv[s][kk], acc[i][0], 0, 0, 0);
            };
            float d[NS][16];
            f32x16 acc[NS][1];
            if constexpr (TWO) {
                gemm(std::integral_constant<int, 1>(), acc);
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const int ml0 = m0 + i * 32 + 4 * lrow;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        d[i][r] = fmaf(acc[i][0][r], s_scale[1][ml0 + (r & 3) + 8 * (r >> 2)], s_shift[1][ml0 + (r & 3) + 8 * (r >> 2)]);
                }
            }
            gemm(std::integral_constant<int, 0>(), acc);
            // TWO: d stands where the residual values stand (PRE); the pointer only says that there is a residual
            conv_epilogue<NS, 1, false, TWO>(acc, s_scale[0] + m0, s_shift[0] + m0, TWO ? a.out : a.res, a.out, a.act, a.Cout, HW, m0, 0,
                                             lrow, pix_off, pix_ok, true, d);
        }
    }
}

template <bool TWO, int NS>
int launch_e64(const E64Args& a, hipStream_t st) {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    }
    // persistent grid: one workgroup per CU (the resident weights leave no room for a second)
    const long long wgs = (a.tiles + E64_WAVES - 1) / E64_WAVES;
    const unsigned grid = (unsigned)(wgs < cus ? wgs : cus);
    hipLaunchKernelGGL((conv1x1_expand64_kernel<TWO, NS>), dim3(grid), dim3(E64_WAVES * 64), 0, st, a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

// the geometry both entry points serve; a recording group (group.h) keeps the launches of rfx_conv2d_f32
int e64_check(int N, int Cin, int HW, int Cout, int stride, int act) {
    if (N <= 0 || HW <= 0) return RFX_E_ARG;
    if (Cin != E64_K || stride != 1 || Cout <= 0 || Cout % E64_MAXC != 0) return RFX_E_ARG;
    if (Cout > E64_MAXC) return RFX_E_LIMIT;
    if (act != RFX_ACT_NONE && act != RFX_ACT_RELU) return RFX_E_ARG;
    if (rfx_group_recording()) return RFX_E_ARG;
    return RFX_OK;
}

}  // namespace

extern "C" int rfx_conv1x1_expand64_f32(const float* in, const float* wT, const float* scale, const float* shift,
                                        const float* residual, float* out, int N, int Cin, int HW, int Cout, int stride, int act,
                                        void* stream) {
    if (!in || !wT || !out) return RFX_E_ARG;
    if (const int rc = e64_check(N, Cin, HW, Cout, stride, act)) return rc;
    E64Args a{};
    a.in[0] = in; a.wT[0] = wT; a.scale[0] = scale; a.shift[0] = shift;
    a.res = residual; a.out = out; a.HW = HW; a.Cout = Cout; a.act = act;
    a.P = (long long)N * HW;
    a.tiles = (a.P + E64_PIX - 1) / E64_PIX;
    return launch_e64<false, E64_PLAIN_NS>(a, rfx_stream(stream));
}

extern "C" int rfx_conv1x1_expand64_dual_f32(const float* in_a, const float* wT_a, const float* scale_a, const float* shift_a,
                                             const float* in_b, const float* wT_b, const float* scale_b, const float* shift_b,
                                             float* out, int N, int Cin, int HW, int Cout, int stride, void* stream) {
    if (!in_a || !wT_a || !in_b || !wT_b || !out) return RFX_E_ARG;
    if (const int rc = e64_check(N, Cin, HW, Cout, stride, RFX_ACT_RELU)) return rc;
    E64Args a{};
    a.in[0] = in_a; a.wT[0] = wT_a; a.scale[0] = scale_a; a.shift[0] = shift_a;
    a.in[1] = in_b; a.wT[1] = wT_b; a.scale[1] = scale_b; a.shift[1] = shift_b;
    a.res = nullptr; a.out = out; a.HW = HW; a.Cout = Cout; a.act = RFX_ACT_RELU;
    a.P = (long long)N * HW;
    a.tiles = (a.P + E64_PIX - 1) / E64_PIX;
    return launch_e64<true, E64_DUAL_NS>(a, rfx_stream(stream));
}
