// conv1x1s.hip -- 1x1 / stride 1 convolution (+ folded BatchNorm, residual, ReLU) with float32 results on the bf16 matrix pipe by
// EXACT operand splitting (the Bottleneck conv1 / conv3 layers of the ResNet-50 trunk, model/resnet50.py:71-79,93-103).  The scheme,
// its numerics and the operand layouts: conv_split.h (read its header first).
//
// Weights: the packed pieces wS[kb = k / 16][piece][h][m (Mpad)][8 bf16].  Activations: a workgroup's staging threads load 8
// consecutive k of one pixel (8 dwords, a wavefront = 64 consecutive pixels = 256 contiguous bytes per load), split them (once per
// workgroup) and store three 16-byte words into the LDS image
//     Bs[piece][h][pixel (128)][8 bf16]
// so that both fragments of an MFMA are single conflict-free ds_read_b128 (consecutive lanes, consecutive words).
// One 16-k block per stage, LDS double buffered, one barrier per stage: registers hold block s+1 while block s runs on the matrix
// pipe and block s+2 is in flight.  Every wavefront owns 32 TM channels x 64 pixels; two tiles:
//   * 64 TM channels x 128 pixels, 2 x 2 wavefronts (conv1x1_split_kernel<TM>): TM = 1 for Cout <= 64, TM = 2 otherwise;
//   * 256 channels x 128 pixels, 4 x 2 wavefronts on 512 threads (conv1x1_split_wide_kernel): the SAME 128-pixel activation image per
//     stage under twice the matrix work -- the activation loads, the split and the Bs writes per MFMA halve (each thread stages 4 k
//     of a pixel instead of 8), a layer with Cout <= 256 reads and splits its input exactly once, a 1024-channel layer 4 times
//     instead of 8.  74 KB of LDS: one workgroup per CU, the same 2 wavefronts per SIMD as two 128-channel workgroups.  Taken where
//     Cout >= 256, Cin >= 512 and the launch's rounds over the CUs come out shorter (c1s_tile_channels; RFX_C1S_WIDE=0: never).
// Only the assignment of tiles to wavefronts differs: every output element sees the same 16-k blocks in the same order, the same six
// products per block into the same two accumulators, one acc += low and the same epilogue -- the tiles agree bit for bit.
#include "common.h"
#include "conv_epilogue.h"
#include "conv_split.h"
#include "conv_tile.h"
#include "group.h"

namespace {

struct C1SArgs {
    const float* in; const u32x4* wS; const float* scale; const float* shift; const float* res; float* out;
    int Cin, HW, Cout, act, Mpad;      // HW: OUTPUT pixels per image
    long long P;   // N*HW
    int tilesM, tilesP;
    int stride, Win, Wo, HWin;         // stride 2 (the projection shortcuts, model/resnet50.py:139-143): input pixel (2y, 2x) of a Win-wide map
};

// WM wavefronts along the channels x 2 along the pixels, each with a 32 TM x 64 output: <1, 2> / <2, 2> = 64 / 128 channels on 256
// threads, <2, 4> = the wide tile, 256 channels on 512 threads over the SAME 128-pixel activation image.
template <int TM, int WM>
__device__ __forceinline__ void conv1x1_split_body(const C1SArgs& a, const unsigned bx, const unsigned) {
    constexpr int BM = 32 * TM * WM, BN = 128, KB = 16, NT = 128 * WM;
    constexpr bool WIDE = WM == 4;
    __shared__ u32x4 As[2][3][2][BM];                   // a stage's weight image: 384 / 768 / 1536 words
    __shared__ u32x4 Bs[2][3][2][BN];
    __shared__ float s_scale[BM], s_shift[BM];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = lane >> 5, lcol = lane & 31;
    const size_t HW = (size_t)a.HW, HWin = (size_t)a.HWin;
    const int nk = a.Cin / KB;

    // tile -> (m0, n0), m-tile fastest (the workgroups that share one pixel tile sit on one L2)
    const int bid = xcd_remap(bx, a.tilesM * a.tilesP);
    const int m0 = (bid % a.tilesM) * BM;
    const long long n0 = (long long)(bid / a.tilesM) * BN;
    // staging roles.  A: the last wide tile of a Cout in (256 j, 256 j + 128] ends 128 rows past Mpad
    SplitWeights<BM, NT> wa;
    wa.init(a.wS, a.Mpad, m0, WIDE);
    // B: thread = (q = t >> 7, pixel t & 127): rows k0 + NB q .. + NB - 1 of that pixel, NB = 8 (256 threads: one 16-byte word of
    // each piece) or 4 (512 threads: one half of it -- every wavefront loads and splits the same share, no branch around the loads)
    constexpr int NB = 2048 / NT;
    const int bh = t >> 7, bp = t & 127;
    const float* bsrc;
    {
        long long p = n0 + bp;
        if (p >= a.P) p = a.P - 1;                                                  // columns past the end: any valid address
        const long long n = p / a.HW;
        int off = (int)(p - n * a.HW);
        if (a.stride != 1) { const int y = off / a.Wo, x = off - y * a.Wo; off = y * a.stride * a.Win + x * a.stride; }
        bsrc = a.in + ((size_t)n * a.Cin + NB * bh) * HWin + (size_t)off;                         // + k0 * HWin
    }
    float rb[NB];
    auto load_stage = [&](int kb) {
        wa.load(kb, a.Mpad);
#pragma unroll
        for (int i = 0; i < NB; ++i) rb[i] = bsrc[(size_t)(kb * KB + i) * HWin];
    };
    auto store_stage = [&](int buf) {
        wa.store(&As[buf][0][0][0]);
        if constexpr (NB == 8) {
            u32x4 hi, mid, lo;
            split_word(rb, hi, mid, lo);
            Bs[buf][0][bh][bp] = hi;
            Bs[buf][1][bh][bp] = mid;
            Bs[buf][2][bh][bp] = lo;
        } else {                                            // k half bh >> 1, 8-byte half bh & 1 of its word
            u32x2 hi, mid, lo;
            split_word(rb, hi, mid, lo);
            u32x2* w = reinterpret_cast<u32x2*>(&Bs[buf][0][bh >> 1][bp]) + (bh & 1);
            w[0] = hi;
            w[4 * BN] = mid;                                // one piece = 2 * BN words of two halves
            w[8 * BN] = lo;
        }
    };
    stage_bn<BM>(s_scale, s_shift, a.scale, a.shift, m0, a.Cout);
    load_stage(0);
    store_stage(0);
    if (nk > 1) load_stage(1);
    __syncthreads();

    f32x16 acc[TM][2], low[TM][2];
    acc_zero(acc);
    acc_zero(low);

    for (int s = 0; s < nk; ++s) {
        const int cur = s & 1;
        // fragments of block s: A rows wm*TM*32 + i*32 + lcol, B pixels wn*64 + j*32 + lcol, k half lrow
        bf16x8 af[3][TM], bf[3][2];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
#pragma unroll
            for (int i = 0; i < TM; ++i) af[pc][i] = as_frag(As[cur][pc][lrow][wm * TM * 32 + i * 32 + lcol]);
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[pc][j] = as_frag(Bs[cur][pc][lrow][wn * 64 + j * 32 + lcol]);
        }
        if (s + 1 < nk) store_stage(cur ^ 1);          // block s+1: registers -> the other buffer (its readers passed the last barrier)
        if (s + 2 < nk) load_stage(s + 2);
        __builtin_amdgcn_sched_barrier(0);
        // smallest terms first into the low accumulator; hi*hi alone in the main one
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                low[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2][i], bf[0][j], low[i][j], 0, 0, 0);    // lo  * hi
                low[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[2][j], low[i][j], 0, 0, 0);    // hi  * lo
                low[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][i], bf[1][j], low[i][j], 0, 0, 0);    // mid * mid
            }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                low[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][i], bf[0][j], low[i][j], 0, 0, 0);    // mid * hi
                low[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[1][j], low[i][j], 0, 0, 0);    // hi  * mid
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bf[0][j], acc[i][j], 0, 0, 0);    // hi  * hi
            }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
    }
    acc_add(acc, low);

    size_t pix_off[2];
    bool pix_ok[2];
    pix_linear<2>(pix_off, pix_ok, n0 + wn * 64 + lcol, a.P, a.HW, a.Cout);
    conv_epilogue<TM, 2, false>(acc, s_scale, s_shift, a.res, a.out, a.act, a.Cout, HW, m0, wm, lrow, pix_off, pix_ok, m0 + BM <= a.Cout);
}

template <int TM> using Split1 = RfxFamily<C1SArgs, conv1x1_split_body<TM, 2>, 256, 2>;
// the wide tile: 74 KB of LDS, one workgroup of 8 wavefronts per CU -- 2 wavefronts per SIMD, as two 256-thread workgroups have
using Split1Wide = RfxFamily<C1SArgs, conv1x1_split_body<2, 4>, 512, 1>;

template <int TM>
__global__ __launch_bounds__((Split1<TM>::BLOCK), (Split1<TM>::min_waves())) void conv1x1_split_kernel(C1SArgs a) {
    conv1x1_split_body<TM, 2>(a, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(Split1Wide::BLOCK, Split1Wide::min_waves()) void conv1x1_split_wide_kernel(C1SArgs a) {
    conv1x1_split_body<2, 4>(a, blockIdx.x, gridDim.x);
}

// Channels per workgroup tile of a launch: 64 (Cout <= 64), 128, or 256 where the wide tile is the faster one.  Measured (MI355X,
// scripts/ubench/split_bench.py --c1s-ab, profiles/c1s_wide_ab.json):
//   * a wide workgroup has its CU to itself, so its epilogue (residual loads, stores) overlaps no other workgroup's K loop: with
//     Cin <= 256 the wide tile is level with or behind the 128-channel one (256 -> 1024 + residual 1.01x / 0.95x / 0.92x at 60x80 /
//     25x33 / 15x20, 128 -> 512 0.97x), from Cin = 512 on it is 4 - 11 % faster on full launches -> Cin >= 512 only;
//   * workgroup times at K = 512 (K = 1024 alike): one 128-channel workgroup alone on its CU 0.031 ms, two of them sharing it
//     0.053 ms, one wide one 0.043 ms = 0.58 : 1 : 0.81.  A launch takes its rounds over the CUs: W wide workgroups
//     ceil(W / CUs) * 0.81; the 2 W 128-channel ones 1 per full round of 2 CUs workgroups, plus 0.58 for a rest of at most one per
//     CU or 1 for a larger rest.  The rule takes the cheaper side; it reproduces every measured winner (W = 150, 207, 413, >= 1200
//     wide; W = 38, 75, 300 not).  Large launches always come out wide; the small pyramid levels and late multi-homography rounds
//     mostly stay on 128 channels.
// RFX_C1S_WIDE (read once): 0 = never the wide tile, 1 = wherever Cout >= 256 (A/B runs and tests).
int c1s_tile_channels(long long P, int Cin, int Cout) {
    static const int mode = [] { const char* e = getenv("RFX_C1S_WIDE"); return e ? (atoi(e) == 0 ? 0 : 1) : -1; }();
    static const long long cus = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return (long long)(n > 0 ? n : 256);
    }();
    if (Cout <= 64) return 64;
    if (Cout < 256 || mode == 0) return 128;
    if (mode == 1) return 256;
    if (Cin < 512) return 128;
    const long long tp = (P + 127) / 128, w = (Cout + 255) / 256 * tp, n = (Cout + 127) / 128 * tp;
    const long long rest = n % (2 * cus);
    const long long cost_wide = (w + cus - 1) / cus * 81, cost_128 = n / (2 * cus) * 100 + (rest == 0 ? 0 : rest <= cus ? 58 : 100);
    return cost_wide < cost_128 ? 256 : 128;
}

template <int TM, int WM>
int launch_split(C1SArgs& a, hipStream_t st) {
    constexpr int BM = 32 * TM * WM;
    a.tilesM = (a.Cout + BM - 1) / BM;
    a.tilesP = (int)((a.P + 127) / 128);
    const long long nwg = (long long)a.tilesM * a.tilesP;
    if (nwg > 0x7fffffffLL) return RFX_E_LIMIT;
    if constexpr (WM == 4) return Split1Wide::launch(conv1x1_split_wide_kernel, a, (unsigned)nwg, st);
    else return Split1<TM>::launch(conv1x1_split_kernel<TM>, a, (unsigned)nwg, st);
}

}  // namespace

static int conv1x1_split_launch(const float* in, const void* wS, const float* scale, const float* shift, const float* residual,
                                float* out, int N, int Cin, int Hin, int Win, int Cout, int stride, int act, void* stream) {
    if (const int rc = conv_check_common(in, wS, out, N, Cin, Hin, Win, Cout, act)) return rc;
    if (stride != 1 && stride != 2) return RFX_E_ARG;
    const int Ho = (Hin - 1) / stride + 1, Wo = (Win - 1) / stride + 1;
    C1SArgs a;
    a.in = in; a.wS = reinterpret_cast<const u32x4*>(wS); a.scale = scale; a.shift = shift; a.res = residual; a.out = out;
    a.Cin = Cin; a.HW = Ho * Wo; a.Cout = Cout; a.act = act; a.Mpad = (Cout + 127) / 128 * 128;
    a.P = (long long)N * a.HW;
    a.stride = stride; a.Win = Win; a.Wo = Wo; a.HWin = Hin * Win;
    switch (c1s_tile_channels(a.P, Cin, Cout)) {
        case 256: return launch_split<2, 4>(a, rfx_stream(stream));
        case 128: return launch_split<2, 2>(a, rfx_stream(stream));
        default: return launch_split<1, 2>(a, rfx_stream(stream));
    }
}

extern "C" int rfx_conv1x1_split_tile_channels(int N, int Cin, int HWout, int Cout) {
    if (N <= 0 || Cin <= 0 || HWout <= 0 || Cout <= 0) return RFX_E_ARG;
    return c1s_tile_channels((long long)N * HWout, Cin, Cout);
}

extern "C" int rfx_conv1x1_split_f32(const float* in, const void* wS, const float* scale, const float* shift, const float* residual,
                                     float* out, int N, int Cin, int HW, int Cout, int act, void* stream) {
    return conv1x1_split_launch(in, wS, scale, shift, residual, out, N, Cin, 1, HW, Cout, 1, act, stream);
}

extern "C" int rfx_conv1x1_split_strided_f32(const float* in, const void* wS, const float* scale, const float* shift, const float* residual,
                                             float* out, int N, int Cin, int Hin, int Win, int Cout, int stride, int act, void* stream) {
    return conv1x1_split_launch(in, wS, scale, shift, residual, out, N, Cin, Hin, Win, Cout, stride, act, stream);
}
