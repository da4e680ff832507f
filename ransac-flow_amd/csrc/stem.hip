// stem.hip -- the two fused network stems.  Both kernels follow one scheme: a workgroup owns a tile of POOLED outputs for ALL output
// channels, stages the input patch under the tile in LDS once, and walks the 32-channel groups over it in a rolled loop:
//   MFMA phase (fp32 32x32x2, one chain per output, k ascending in pairs (2kk, 2kk+1): the accumulators are bit-identical to
//   conv.hip's) -> BN + ReLU -> LDS tile -> barrier -> pooling pass -> barrier -> next group.
// A group's weights (and, in the 3x3 stem, its BN vectors) are dead after its MFMA phase: the next group's are requested at the
// top of the pooling pass and land under it.  The LDS tile is reused by the groups in turn (hence the second barrier).
//
// FeatureExtractor stem (model/model.py:68-72, forward :106-110):
//     conv3x3(3 -> 64, stride 1, pad 1) -> BatchNorm (folded) -> ReLU -> MaxPool2d(2, stride 1) -> BlurPool(stride 2)
// Un-fused, the 64-channel full-resolution map (480 x 640 x 64 floats per image: the largest tensor of the whole
// pipeline, 10 GB for a batch of 128 images) is written by the convolution and read back by the pooling kernel; both
// are bound by exactly that traffic.  Here a workgroup owns a 4 x 16 tile of pooled outputs:
//   1. the 3 x 12 x 36 input patch it needs goes to LDS (zero filled outside the image = the conv padding), once per tile;
//   2. per channel group the 10 x 34 conv outputs under the tile are computed on the fp32 MFMA: pixel p = row*34 + col is a
//      column of the 32x32 tile, k = c*9 + kh*3 + kw (27, padded to 28); B operands are single ds_read_b32 from the patch at
//      per-lane addresses;
//   3. fma(acc, scale, shift) -> ReLU -> LDS tile [32 ch][10][34];
//   4. max 2x2 / blur [1 2 1]^2/16 stride 2 with ReflectionPad2d(1) on the max-pooled map, in the operation order of
//      maxblurpool2d_kernel (pool.hip) -> bit-identical to conv2d + maxblurpool2d; a thread produces 2x2 blocks of
//      outputs from a 6x6 window (border blocks take the per-output path that reflects indices).
// Only the /2 map is written: HBM traffic per image drops from (3 + 64 + 64 + 16) to (3 + 16) full-resolution planes.
#include "common.h"
#include "group.h"

namespace {

constexpr int TH = 4, TW = 16;                 // pooled outputs per workgroup
constexpr int CR = 2 * TH + 2, CC = 2 * TW + 2; // conv outputs under the tile: 10 x 34
constexpr int PRW = CR + 2, PCL = CC + 2;       // input patch 12 x 36
constexpr int CST = CC + 1;                     // row stride of the conv tile in LDS (35: odd -> rows on different banks)
constexpr int CPS = CR * CST + 1;               // channel-plane stride 351: ODD, so the four channels a wavefront of the pooling pass covers
                                                // (8 blocks x 2 block rows x 4 channels, block columns 4 words apart) fall into the four bank
                                                // classes mod 4 -- every bank twice, the minimum for 64 lanes; 350 gave two classes: 4-way
                                                // conflicts on each of the 36 window reads (SQ_LDS_BANK_CONFLICT 0.20 per instruction, round 6)
constexpr int NPX = CR * CC;                    // 340 conv pixels
constexpr int NSUB = (NPX + 31) / 32;           // 11 MFMA sub-tiles of 32 pixels
constexpr int KKS = 14;                         // 28 = 27 padded k, as k-pairs
constexpr int MCH = 32;                         // channels per group (one MFMA tile of rows)

struct StemArgs {
    const float* in; const float* wT; const float* scale; const float* shift; float* out;
    int N, H, W, Cout, Mpad, Ho, Wo, tilesH, tilesW, chGroups;
};

__device__ __forceinline__ int reflect1i(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// The pooled values are ReLU outputs: +0, positive, +inf or NaN.  For such floats the IEEE order is the order of the bit
// patterns as unsigned integers and every NaN pattern lies above +inf, so an unsigned integer max IS the NaN-propagating
// float max of MaxPool2d (which NaN payload survives is the only freedom) -- 1 instruction instead of 4 per comparison.
__device__ __forceinline__ float umaxf(float x, float y) {
    const unsigned a = __float_as_uint(x), b = __float_as_uint(y);
    return __uint_as_float(a > b ? a : b);
}

__device__ __forceinline__ void stem_conv_maxblur_body(const StemArgs& a, const unsigned bx, const unsigned) {
    __shared__ float P[3][PRW][PCL];          // input patch
    __shared__ float C[MCH * CPS];            // conv + BN + ReLU outputs of ONE channel group under the tile: [channel][CR][CST], planes CPS apart

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lrow = lane >> 5, lcol = lane & 31;
    int bid = (int)bx;                                        // one workgroup per pooled tile, all channel groups
    const int tw = bid % a.tilesW; bid /= a.tilesW;
    const int th = bid % a.tilesH;
    const int n = bid / a.tilesH;
    const int oh0 = th * TH, ow0 = tw * TW;
    const int cy0 = 2 * oh0 - 1, cx0 = 2 * ow0 - 1;           // first conv row / column under the tile (= first max-map row / column)
    const size_t HW = (size_t)a.H * a.W;

    // ---- 1. input patch (rows cy0-1 .. cy0+10, cols cx0-1 .. cx0+34), zero outside the image
    const float* inn = a.in + (size_t)n * 3 * HW;
    constexpr int NP = (3 * PRW * PCL + 255) / 256;   // 6 patch elements per thread
    float pv_[NP];
    bool pok[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {   // all loads first, masks afterwards: a select on a load in flight would wait for it
        const int idx = t + 256 * u;
        const int c = idx / (PRW * PCL), rem = idx - c * (PRW * PCL);
        const int pr = rem / PCL, pc = rem - pr * PCL;
        const int gy = cy0 - 1 + pr, gx = cx0 - 1 + pc;
        pok[u] = idx < 3 * PRW * PCL && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        pv_[u] = inn[pok[u] ? (size_t)c * HW + (size_t)gy * a.W + gx : 0];
    }
    // A operand of this lane for one channel group: weights of channel m0 + lcol for k = 2kk + lrow (rows K..Kpad-1 of wT are zero)
    float af[KKS];
    auto load_weights = [&](const int m0) {
#pragma unroll
        for (int kk = 0; kk < KKS; ++kk) af[kk] = a.wT[(size_t)(2 * kk + lrow) * a.Mpad + m0 + lcol];
    };
    load_weights(0);                                  // in flight while the patch goes to LDS
    // per-lane patch offsets of the 14 k-pairs (tap (c, kh, kw) of k = 2kk + lrow); k = 27 is the zero pad
    int koff[KKS];
#pragma unroll
    for (int kk = 0; kk < KKS; ++kk) {
        const int k = 2 * kk + lrow;
        const int c = k / 9, t9 = k - c * 9, kh = t9 / 3, kw = t9 - kh * 3;
        koff[kk] = k < 27 ? c * (PRW * PCL) + kh * PCL + kw : 0;
    }
#pragma unroll
    for (int u = 0; u < NP; ++u)
        if (t + 256 * u < 3 * PRW * PCL) (&P[0][0][0])[t + 256 * u] = pok[u] ? pv_[u] : 0.0f;
    __syncthreads();

    const float* pf = &P[0][0][0];
    const float w3[3] = {0.25f, 0.5f, 0.25f};
    const int Hm = a.H - 1, Wm = a.W - 1;
#pragma unroll 1
    for (int cg = 0; cg < a.chGroups; ++cg) {
    const int m0 = cg * MCH;
    // folded-BN vectors of this lane's 16 accumulator rows: requested here, first used after the first MFMA chain (prefetched
    // with the weights they would stay live across the pooling pass and cost the third resident workgroup)
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ch = m0 + 4 * lrow + (r & 3) + 8 * (r >> 2);
        sc[r] = a.scale ? a.scale[ch] : 1.0f;
        sh[r] = a.shift ? a.shift[ch] : 0.0f;
    }
    // ---- 2./3. conv on the MFMA, BN + ReLU, tile -> LDS
    for (int s = wave; s < NSUB; s += 4) {
        const int p = s * 32 + lcol;
        const bool pv = p < NPX;
        const int pc = pv ? p : 0;
        const int py = pc / CC, px = pc - py * CC;
        int pbase = py * PCL + px;
        asm volatile("" : "+v"(pbase));               // the 14 B addresses are the same for every channel group: formed here, not
                                                      // hoisted out of the group loop into 14 registers per sub-tile
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < KKS; ++kk) {
            float b = pf[pbase + koff[kk]];
            if (kk == KKS - 1) b = lrow ? 0.0f : b;   // k = 27: padded tap
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], b, acc, 0, 0, 0);
        }
        if (pv) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = fmaf(acc[r], sc[r], sh[r]);
                v = v > 0.0f ? v : 0.0f;
                C[(4 * lrow + (r & 3) + 8 * (r >> 2)) * CPS + py * CST + px] = v;
            }
        }
    }
    __syncthreads();
    if (cg + 1 < a.chGroups) load_weights(m0 + MCH);  // af is dead until the next group's MFMA phase: lands under the pooling pass

    // ---- 4. max 2x2 (stride 1) + blur/2 with reflection on the max-pooled map; 2x2 output blocks
    for (int b = t; b < MCH * (TH / 2) * (TW / 2); b += 256) {
        const int bx = b % (TW / 2), by = (b / (TW / 2)) % (TH / 2), ch = b / ((TW / 2) * (TH / 2));
        const int oh = oh0 + 2 * by, ow = ow0 + 2 * bx;        // first output of the block
        if (oh >= a.Ho || ow >= a.Wo) continue;
        float* dst = a.out + ((size_t)n * a.Cout + m0 + ch) * a.Ho * a.Wo;
        const float* Cc = C + ch * CPS;
        // interior: the 5x5 max-map window rows 2oh-1 .. 2oh+3, cols 2ow-1 .. 2ow+3 needs no reflection
        const bool interior = oh >= 1 && 2 * oh + 3 <= Hm - 1 && ow >= 1 && 2 * ow + 3 <= Wm - 1 && oh + 1 < a.Ho && ow + 1 < a.Wo;
        if (interior) {
            const int ly = 2 * oh - 1 - cy0, lx = 2 * ow - 1 - cx0;   // = 4*by, 4*bx
            float v[6][6];
#pragma unroll
            for (int y = 0; y < 6; ++y)
#pragma unroll
                for (int x = 0; x < 6; ++x) v[y][x] = Cc[(ly + y) * CST + lx + x];
            float hmx[5][6], M[5][5];   // separable: vertical pair max, then horizontal pair max
#pragma unroll
            for (int y = 0; y < 5; ++y)
#pragma unroll
                for (int x = 0; x < 6; ++x) hmx[y][x] = umaxf(v[y][x], v[y + 1][x]);
#pragma unroll
            for (int y = 0; y < 5; ++y)
#pragma unroll
                for (int x = 0; x < 5; ++x) M[y][x] = umaxf(hmx[y][x], hmx[y][x + 1]);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    float acc = 0.0f;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) acc = fmaf(M[2 * dy + i][2 * dx + j], w3[i] * w3[j], acc);
                    dst[(size_t)(oh + dy) * a.Wo + ow + dx] = acc;
                }
            continue;
        }
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int o_h = oh + dy, o_w = ow + dx;
                if (o_h >= a.Ho || o_w >= a.Wo) continue;
                float acc = 0.0f;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int my = reflect1i(2 * o_h - 1 + i, Hm) - cy0;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int mx = reflect1i(2 * o_w - 1 + j, Wm) - cx0;
                        const float m = umaxf(umaxf(Cc[my * CST + mx], Cc[(my + 1) * CST + mx]), umaxf(Cc[my * CST + mx + 1], Cc[(my + 1) * CST + mx + 1]));
                        acc = fmaf(m, w3[i] * w3[j], acc);
                    }
                }
                dst[(size_t)o_h * a.Wo + o_w] = acc;
            }
    }
    __syncthreads();                                  // the next group overwrites C
    }
}

using Stem3 = RfxFamily<StemArgs, stem_conv_maxblur_body, 256>;
__global__ __launch_bounds__(Stem3::BLOCK) void stem_conv_maxblur_kernel(StemArgs a) {
    stem_conv_maxblur_body(a, blockIdx.x, gridDim.x);
}


// ---------------------------------------------------------------------------------------------------------------
// ResNet-50 stem (model/resnet50.py:115-120, forward :157-160 as sliced by quick_start/coarseAlignFeatMatch.py:38-41):
//     conv7x7(3 -> 64, stride 2, pad 3) -> BatchNorm (folded) -> ReLU -> MaxPool2d(3, stride 2, pad 1)
// A workgroup owns TH x 16 = 5 x 16 pooled outputs for all channels.  The 3 x 27 x 71 input patch under the 11 x 33 conv outputs
// of the tile is staged in LDS ONCE; every 32-channel group then runs over it (k = c*49 + kh*7 + kw, 147 padded to 148, same
// order and pairing as the implicit-GEMM kernel -> bit-identical accumulators).
// The stride-2 taps of 32 consecutive conv pixels would hit every second LDS word (2-way bank conflicts): the patch
// rows are stored de-interleaved, [even columns | odd columns], so a lane's tap (kh, kw) sits at
// parity(kw)*36 + px + kw/2 and consecutive pixels read consecutive words.
// MFMA sub-tiles are ROW-ALIGNED: sub-tile s < 11 = conv row s, columns 0..31 (32 consecutive LDS words per tap: no bank conflict).
// The HORIZONTAL half of the 3x3 max is taken in registers before anything goes to LDS: after BN + ReLU a lane holds 16 channels
// of conv column lcol; positions outside the conv map become 0 (the identity of the max on ReLU outputs, see umaxf), and two DPP
// row shifts give lane 2*owl the max over columns 2*owl .. 2*owl+2.  A DPP row is 16 lanes, so pooled columns 7 and 15 lack conv
// columns 16 and 32: the twelfth sub-tile computes exactly those two columns for the 11 rows (lanes 0..10: column 16 again -- the
// same chain, the same bits; lanes 16..26: column 32) into a small side array.  Only the 16 pooled columns of a row are stored:
// the tile is [32][11][16] floats (22.5 KB instead of 56 KB) and the pooling pass reads 3 values (6 for pooled columns 7 and 15)
// instead of 9.  The integer max is associative and commutative, so the result has the same bits (NaN payload included) as the
// 9-value loop of maxpool2d_kernel.
// History (scripts/ubench/stem_bench.py; TFLOP/s at 64 x 960x1280 .. 240x320):
//   round 5  TH = 4, one workgroup per (tile, channel group), 9-read pooling                                  54-55
//   round 6  TH = 5 (12 sub-tile slots, 3 per wave)                                                           56-62
//   round 6  both channel groups as two inlined bodies: 150 registers spilled                                 40-50 (dropped)
//   this form: profiles/stem_tiles_ab.json
namespace r50 {
constexpr int TH = 5, TW = 16;
constexpr int CR = 2 * TH + 1, CC = 2 * TW + 1;    // 11 x 33 conv outputs
constexpr int PR = 2 * CR + 5, PCW = 2 * CC + 5;   // 27 x 71 input patch
constexpr int PHALF = 36, PST = 2 * PHALF + 2;     // de-interleaved row: 36 even + 36 odd columns (+2: the lanes of the column
                                                   // sub-tile below sit 2*PST = 148 words apart = 20 banks)
// horizontally reduced tile in LDS: [channel][conv row][pooled column], rows 16 words, planes HPS = 180 words apart (the two lane
// halves of a store are 4 channels = 720 words = 16 banks apart: the 2 x 16 active lanes hit 32 different banks)
constexpr int HPS = CR * TW + 4;
constexpr int SPS = 24;                            // side array [channel][2][12]: conv columns 16 and 32 of the 11 rows
constexpr int NSUB = CR + 1;                       // 11 row sub-tiles + 1 sub-tile for columns 16 and 32
constexpr int KKS = 74;                            // 148 / 2
constexpr int MCH = 32;
__host__ __device__ constexpr int koff(int k) {    // patch offset of tap k = c*49 + kh*7 + kw
    return k >= 147 ? 0 : (k / 49) * (PR * PST) + ((k % 49) / 7) * PST + (((k % 49) % 7) & 1) * PHALF + (((k % 49) % 7) >> 1);
}
}  // namespace r50

struct Stem7Args {
    const float* in; const float* wT; const float* scale; const float* shift; float* out;
    int N, H, W, Cout, Mpad, Hc, Wc, Hp, Wp, tilesH, tilesW, chGroups;
#ifdef RFX_TRACE
    long long* trace;      // experiments only (make trace): 8 words per workgroup (scripts/dbg/stem_trace.py)
#endif
};
// make trace: shader-clock stamps of thread 0.  Words per workgroup: 0 start | 1 patch in LDS | 2 after the barrier | 3 sum over
// the channel groups of MFMA phase + tile stores + barrier | 4 sum of pooling pass + stores + barrier | 5 end | 6 channel groups
#ifdef RFX_TRACE
extern "C" long long* rfx_debug_trace_ptr();
#define RFX_NOW7() ((long long)__builtin_amdgcn_s_memtime())
#define RFX_STAMP7(i) do { if (threadIdx.x == 0 && a.trace) a.trace[(size_t)bx * 8 + (i)] = RFX_NOW7(); } while (0)
#define RFX_PUT7(i, v) do { if (threadIdx.x == 0 && a.trace) a.trace[(size_t)bx * 8 + (i)] = (v); } while (0)
#define RFX_TRACE7(x) x
#else
#define RFX_STAMP7(i)
#define RFX_PUT7(i, v)
#define RFX_TRACE7(x)
#endif

// row_shl:n of the 16-lane DPP row: lane i receives lane i + n of its row, 0 where that leaves the row
template <int N>
__device__ __forceinline__ unsigned row_shl0(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + N, 0xf, 0xf, true);
}

__device__ __forceinline__ void stem7_conv_maxpool_body(const Stem7Args& a, const unsigned bx, const unsigned) {
    constexpr int TH = r50::TH, TW = r50::TW, CR = r50::CR, PR = r50::PR, PCW = r50::PCW, PHALF = r50::PHALF,
                  PST = r50::PST, HPS = r50::HPS, SPS = r50::SPS, NSUB = r50::NSUB, KKS = r50::KKS, MCH = r50::MCH;
    using r50::koff;
    __shared__ float P[3][PR][PST];
    __shared__ float Hx[MCH * HPS];       // max over conv columns 2*owl .. 2*owl+2 (without columns 16 / 32 for owl = 7 / 15)
    __shared__ float Sd[MCH * SPS];       // conv columns 16 and 32
    __shared__ float s_bn[2][128];        // folded-BN vectors (32 registers less across the MFMA loop)

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lrow = lane >> 5, lcol = lane & 31;
    int bid = (int)bx;                                        // one workgroup per pooled tile, all channel groups
    const int tw = bid % a.tilesW; bid /= a.tilesW;
    const int th = bid % a.tilesH;
    const int n = bid / a.tilesH;
    const int oh0 = th * TH, ow0 = tw * TW;
    const int cy0 = 2 * oh0 - 1, cx0 = 2 * ow0 - 1;          // first conv row / column under the tile
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;          // first input row / column of the patch
    const size_t HW = (size_t)a.H * a.W;

    RFX_STAMP7(0);
    // ---- input patch -> registers
    const float* inn = a.in + (size_t)n * 3 * HW;
    constexpr int NP = (3 * PR * PCW + 255) / 256;
    float pv_[NP];
    unsigned pok = 0;
    // element t + 256u of the 3 x 27 x 71 patch: (c, pr, pc) advanced incrementally (256 = 3*71 + 43), no divisions
    const int c_0 = t / (PR * PCW), rem_0 = t - c_0 * (PR * PCW), pr_0 = rem_0 / PCW, pc_0 = rem_0 - pr_0 * PCW;
    {
        int c = c_0, pr = pr_0, pc = pc_0;
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int gy = iy0 + pr, gx = ix0 + pc;
            const bool ok = c < 3 && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
            pok |= ok ? (1u << u) : 0u;
            pv_[u] = inn[ok ? (size_t)c * HW + (size_t)gy * a.W + gx : 0];
            pc += 256 % PCW; pr += 256 / PCW;
            if (pc >= PCW) { pc -= PCW; ++pr; }
            if (pr >= PR) { pr -= PR; ++c; }
        }
    }
    for (int c = t; c < a.Cout && c < 128; c += 256) {
        s_bn[0][c] = a.scale ? a.scale[c] : 1.0f;
        s_bn[1][c] = a.shift ? a.shift[c] : 0.0f;
    }
    // A operand of this lane for one channel group: weights of channel m0 + lcol for k = 2kk + lrow
    float af[KKS];
    // (uniform row pointer + one 32-bit lane offset: 74 scalar-base loads off a single address register)
    auto load_weights = [&](const int m0) {
        const unsigned voff = (unsigned)(lrow * a.Mpad + m0 + lcol);
#pragma unroll
        for (int kk = 0; kk < KKS; ++kk) af[kk] = (a.wT + (size_t)(2 * kk) * a.Mpad)[voff];
    };
    load_weights(0);                       // in flight while the patch goes to LDS
    {
        int c = c_0, pr = pr_0, pc = pc_0;
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            if (c < 3) P[c][pr][(pc & 1) * PHALF + (pc >> 1)] = ((pok >> u) & 1u) ? pv_[u] : 0.0f;
            pc += 256 % PCW; pr += 256 / PCW;
            if (pc >= PCW) { pc -= PCW; ++pr; }
            if (pr >= PR) { pr -= PR; ++c; }
        }
    }
    RFX_STAMP7(1);
    __syncthreads();
    RFX_STAMP7(2);
    RFX_TRACE7(long long tr_mark = RFX_NOW7(); long long tr_mfma = 0; long long tr_pool = 0;)

    const float* pf = &P[0][0][0];
#pragma unroll 1
    for (int cg = 0; cg < a.chGroups; ++cg) {
    const int m0 = cg * MCH;
    // ---- conv on the MFMA, BN + ReLU, horizontal 3-max -> LDS
    for (int s = wave; s < NSUB; s += 4) {
        const bool rowt = s < CR;                                   // wave-uniform
        const int cl = lcol & 15;
        const bool pv = rowt || cl < CR;
        const int py = rowt ? s : (cl < CR ? cl : 0), px = rowt ? lcol : 16 + (lcol & 16);
        int pbase = 2 * py * PST + px;
        asm volatile("" : "+v"(pbase));               // the 74 B addresses are the same for every channel group: formed here, not
                                                      // hoisted out of the group loop into 74 registers per sub-tile
        const bool ok = pv && (unsigned)(cy0 + py) < (unsigned)a.Hc && (unsigned)(cx0 + px) < (unsigned)a.Wc;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < KKS; ++kk) {
            const int off = lrow ? koff(2 * kk + 1) : koff(2 * kk);
            float b = pf[pbase + off];
            if (kk == KKS - 1) b = lrow ? 0.0f : b;   // k = 147: padded tap
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], b, acc, 0, 0, 0);
        }
        if (rowt) {
            unsigned hm[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int chl = m0 + 4 * lrow + (r & 3) + 8 * (r >> 2);
                float v = fmaf(acc[r], s_bn[0][chl], s_bn[1][chl]);
                v = v > 0.0f ? v : 0.0f;
                const unsigned u = ok ? __float_as_uint(v) : 0u;    // outside the conv map: the identity of the max
                const unsigned u1 = row_shl0<1>(u), u2 = row_shl0<2>(u);
                const unsigned m1 = u > u1 ? u : u1;
                hm[r] = m1 > u2 ? m1 : u2;
            }
            if (!(lcol & 1)) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    Hx[(4 * lrow + (r & 3) + 8 * (r >> 2)) * HPS + py * TW + (lcol >> 1)] = __uint_as_float(hm[r]);
            }
        } else if (pv) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int chl = m0 + 4 * lrow + (r & 3) + 8 * (r >> 2);
                float v = fmaf(acc[r], s_bn[0][chl], s_bn[1][chl]);
                v = v > 0.0f ? v : 0.0f;
                Sd[(4 * lrow + (r & 3) + 8 * (r >> 2)) * SPS + (lcol >> 4) * 12 + py] = ok ? v : 0.0f;
            }
        }
    }
    __syncthreads();
    RFX_TRACE7(const long long tr_a = RFX_NOW7(); tr_mfma += tr_a - tr_mark; tr_mark = tr_a;)
    if (cg + 1 < a.chGroups) load_weights(m0 + MCH);    // af is dead until the next group's MFMA phase: lands under the pooling pass

    // ---- the vertical half of MaxPool2d(3, stride 2, pad 1): rows 2*ohl .. 2*ohl+2 of the reduced tile
    for (int o = t; o < MCH * TH * TW; o += 256) {
        const int owl = o % TW, ohl = (o / TW) % TH, ch = o / (TW * TH);
        const int oh = oh0 + ohl, ow = ow0 + owl;
        if (oh >= a.Hp || ow >= a.Wp) continue;
        const float* hx = Hx + ch * HPS + 2 * ohl * TW + owl;
        float m = umaxf(umaxf(hx[0], hx[TW]), hx[2 * TW]);
        if ((owl & 7) == 7) {
            const float* sd = Sd + ch * SPS + (owl >> 3) * 12 + 2 * ohl;
            m = umaxf(m, umaxf(umaxf(sd[0], sd[1]), sd[2]));
        }
        a.out[(((size_t)n * a.Cout + m0 + ch) * a.Hp + oh) * a.Wp + ow] = m;
    }
    __syncthreads();                                    // the next group overwrites Hx / Sd
    RFX_TRACE7(const long long tr_b = RFX_NOW7(); tr_pool += tr_b - tr_mark; tr_mark = tr_b;)
    }
    RFX_PUT7(3, tr_mfma);
    RFX_PUT7(4, tr_pool);
    RFX_STAMP7(5);
    RFX_PUT7(6, (long long)a.chGroups);
}

using Stem7 = RfxFamily<Stem7Args, stem7_conv_maxpool_body, 256, 2>;
__global__ __launch_bounds__(Stem7::BLOCK, Stem7::min_waves()) void stem7_conv_maxpool_kernel(Stem7Args a) {
    stem7_conv_maxpool_body(a, blockIdx.x, gridDim.x);
}

}  // namespace

extern "C" int rfx_stem_conv3x3_maxblur_f32(const float* in, const float* wT, const float* scale, const float* shift,
                                            float* out, int N, int H, int W, int Cout, void* stream) {
    if (!in || !wT || !out || N <= 0 || H < 3 || W < 3 || Cout <= 0) return RFX_E_ARG;
    if (Cout % MCH != 0) return RFX_E_ARG;
    StemArgs a;
    a.in = in; a.wT = wT; a.scale = scale; a.shift = shift; a.out = out;
    a.N = N; a.H = H; a.W = W; a.Cout = Cout; a.Mpad = (Cout + 127) / 128 * 128;
    a.Ho = (H - 2) / 2 + 1; a.Wo = (W - 2) / 2 + 1;
    a.tilesH = (a.Ho + TH - 1) / TH; a.tilesW = (a.Wo + TW - 1) / TW; a.chGroups = Cout / MCH;
    const long long nwg = (long long)N * a.tilesH * a.tilesW;      // a workgroup walks all channel groups of its tile
    if (nwg > 0x7fffffffLL) return RFX_E_LIMIT;
    return Stem3::launch(stem_conv_maxblur_kernel, a, (unsigned)nwg, rfx_stream(stream));
}

extern "C" int rfx_stem_conv7x7_maxpool_f32(const float* in, const float* wT, const float* scale, const float* shift,
                                            float* out, int N, int H, int W, int Cout, void* stream) {
    if (!in || !wT || !out || N <= 0 || H < 1 || W < 1 || Cout <= 0) return RFX_E_ARG;
    if (Cout % r50::MCH != 0) return RFX_E_ARG;
    if (Cout > 128) return RFX_E_LIMIT;                    // folded-BN vectors staged in LDS (s_bn)
    Stem7Args a;
    a.in = in; a.wT = wT; a.scale = scale; a.shift = shift; a.out = out;
    a.N = N; a.H = H; a.W = W; a.Cout = Cout; a.Mpad = (Cout + 127) / 128 * 128;
    a.Hc = (H + 6 - 7) / 2 + 1; a.Wc = (W + 6 - 7) / 2 + 1;
    a.Hp = (a.Hc + 2 - 3) / 2 + 1; a.Wp = (a.Wc + 2 - 3) / 2 + 1;
    a.tilesH = (a.Hp + r50::TH - 1) / r50::TH; a.tilesW = (a.Wp + r50::TW - 1) / r50::TW; a.chGroups = Cout / r50::MCH;
    const long long nwg = (long long)N * a.tilesH * a.tilesW;      // a workgroup walks all channel groups of its tile
    if (nwg > 0x7fffffffLL) return RFX_E_LIMIT;
#ifdef RFX_TRACE
    a.trace = rfx_debug_trace_ptr();
#endif
    return Stem7::launch(stem7_conv_maxpool_kernel, a, (unsigned)nwg, rfx_stream(stream));
}
