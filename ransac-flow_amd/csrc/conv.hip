// conv.hip -- implicit-GEMM fp32 convolution on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Replaces the cuDNN convolutions + eval-mode BatchNorm + ReLU (+ residual add) the reference issues
// for the ResNet-50 conv1..layer3 trunk (model/resnet50.py:68-104,112-169 via
// quick_start/coarseAlignFeatMatch.py:106,124), the FeatureExtractor (model/model.py:27-56,106-115)
// and the NetFlowCoarse / NetMatchability conv stacks (model/model.py:210-226,289-305).
//
// GEMM view (NCHW, no layout change anywhere in the pipeline):
//     D[m][p] = sum_k  W^T[k][m] * im2col[k][p]      m = output channel, p = (n,oh,ow), k = (c,kh,kw)
// A operand = packed weights [Kpad][Mpad] (k-major, zero padded, so tile loads need no guards),
// B operand = input patches gathered on the fly (coalesced along ow), both staged through LDS as
// through LDS; a 32x32x2 MFMA lane supplies one float per operand: lane l holds
// A[m = l&31][k = l>>5] and B[k = l>>5][p = l&31].
// The fp32 MFMA is bit-for-bit a k-ordered fmaf chain, so results are deterministic and within
// fp32 round-off of the reference's cuDNN/oneDNN sums.
//
// Block = 256 threads = 2x2 waves; wave tile = (32*TM) x (32*TN); BK = 32; register-prefetch double
// buffering (global loads of step s+1 are in flight while step s runs on the matrix pipe).  LDS holds each
// operand as [k&1][row][k>>1] so that a lane reads its 16 k-pairs of a step with four ds_read_b128
// (XOR-swizzled 16-byte chunks: conflict free) instead of sixteen ds_read_b32.
// Epilogue fused: y = fma(acc, scale[m], shift[m]) (+ residual) -> ReLU / sigmoid; stores coalesced
// along the pixel dimension (the MFMA C/D column index is the pixel).
#include "common.h"
#include "conv_dispatch.h"
#include "conv_epilogue.h"
#include "conv_tile.h"
#include "group.h"

struct ConvArgs {
    const float* in;
    const float* wT;
    const int32_t* ktab;
    const float* scale;
    const float* shift;
    const float* res;
    float* out;
    int N, Cin, Hin, Win, Cout, Hout, Wout, stride, pad, act;
    int Kpad, Mpad;
    long long P;  // N*Hout*Wout
    int tilesM, tilesP;
#ifdef RFX_TRACE
    long long* trace;  // experiments only (make TRACE=1): 4 wall-clock stamps per workgroup
#endif
};
#ifdef RFX_TRACE
#define RFX_STAMP(i) do { if (tid == 0 && a.trace) a.trace[(size_t)blockIdx.x * 4 + (i)] = wall_clock64(); } while (0)
static long long* g_trace = nullptr;
extern "C" void rfx_debug_trace(long long* p) { g_trace = p; }
extern "C" long long* rfx_debug_trace_ptr() { return g_trace; }
#else
#define RFX_STAMP(i)
#endif

// ONE = 1x1 kernel with pad 0 (any stride): k IS the input channel and every tap is in bounds, so the im2col
// gather needs no ktab decode and no bounds logic (address = pixel base + k * Hin*Win).
// WS = wave-specialised form for long K loops: 512 threads = 4 MFMA wavefronts (one per SIMD, 64x64 outputs each,
// nothing but ds_read_b128 + MFMA in their loop) + 4 loader wavefronts (one per SIMD) that run the whole im2col
// gather / weight fetch / LDS staging.  A 32x32x2 fp32 MFMA keeps the matrix pipe busy for 64 cycles per issue,
// so the loader wave's ~600 address/load/store instructions per K step fit in the issue slots the MFMA wave
// leaves free -- the overlap the single-role kernel only gets statistically from a second workgroup.
// VECB (only with ONE, stride 1, Hout*Wout % 4 == 0): a thread fetches 4 consecutive pixels of one input channel
// with one 16-byte load (the im2col row of a 1x1 convolution is the NCHW plane itself), mirroring the weight side:
// 4x fewer gather instructions.
template <int TM, int TN, bool ONE, bool WS, bool VECB>
__device__ __forceinline__ void conv2d_mfma_body(const ConvArgs& a, const unsigned bx, const unsigned) {
    constexpr int BM = 64 * TM, BN = 64 * TN, BK = 32, KK = BK / 2;  // KK k-pairs per step
    constexpr int B_NI = BN / 8;                                      // gathered values per thread per step
    constexpr int A_MG = BM / 4;                                        // groups of 4 consecutive m per tile
    constexpr int A_KQ = 256 / A_MG;                                    // k-roles per m-group (8 or 16)
    constexpr int A_NJ = 32 / A_KQ;                                     // k rows (float4 loads) per thread: 4 or 2
    constexpr int B_PG = BN / 4, B_KQ = 256 / B_PG, B_NJ = 32 / B_KQ;   // the same decomposition for the pixel side (VECB)
    // LDS image per operand: [h = k&1][row (m or pixel)][kk = k>>1], 16 consecutive k-pairs per row, so that a
    // lane fetches its operands for a whole K step with four ds_read_b128.  16-byte chunk q of row r is stored
    // at chunk q ^ ((r>>2)&3): the 16-lane ds_read_b128 service groups then touch 16 distinct bank quads.
    // Round 5, WHICH access conflicts: the A-side (weight) stores below.  A 16-lane group of one store instruction
    // writes rows mg*4 + e, mg = 0..15 -- 256 bytes apart, i.e. the same bank -- at chunk (iA0 >> 2) ^ (mg & 3): FOUR bank quads for
    // 16 lanes, a 4-way conflict on every weight store (the gathered B side writes whole rows: conflict free; all reads are
    // conflict free).  That is the SQ_LDS_BANK_CONFLICT / SQ_ACTIVE_INST_ANY = 0.41-0.48 of round 4's counters.  The cure that
    // needs no second packed weight array -- a K-MAJOR A image As[k][m] (straight 16-byte copies, ds_read_b32 operands, the scheme
    // of conv1x1.hip) -- was built and measured on the layer that still lives here (1x1 / stride 2 projection 256 -> 512 at 120x160,
    // 128 images): 91.7 vs 95.0 TFLOP/s, i.e. 3.5 % SLOWER (profiles/r05_conv_ab.jsonl): 32 ds_read_b32 per K step and wave tile
    // instead of 8 ds_read_b128 cost more issue slots next to the ~10 VALU instructions per gathered B element than the
    // conflicting stores (8 of ~100 LDS instructions per thread and step).  Reverted; the conflicts stay, priced at < 0.2 % of the step.
    __shared__ __attribute__((aligned(16))) float As[2][2][BM][KK];
    __shared__ __attribute__((aligned(16))) float Bs[2][2][BN][KK];
    __shared__ float s_scale[BM], s_shift[BM];

    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3;
    const int t = tid & 255;  // staging index (WS: the loader wavefronts are threads 256..511)
    const int wm = wave >> 1, wn = wave & 1;

    RFX_STAMP(0);
    // m-tile fastest: the blocks that share one im2col pixel tile run on one L2
    const int bid = xcd_remap(bx, a.tilesM * a.tilesP);
    const int tm_idx = bid % a.tilesM;
    const int tp_idx = bid / a.tilesM;
    const int m0 = tm_idx * BM;
    const long long n0 = (long long)tp_idx * BN;

    // folded BatchNorm of this block's output channels -> LDS (visible after the first barrier).  A second copy of stage_bn
    // (conv_tile.h), kept on purpose: through the helper the 64-channel instances allocate 117 / 119 VGPRs where the committed
    // resource table pins 121 / 123
    if (tid < BM) {
        const int m = m0 + t;
        s_scale[t] = (a.scale && m < a.Cout) ? a.scale[m] : 1.0f;
        s_shift[t] = (a.shift && m < a.Cout) ? a.shift[m] : 0.0f;
    }
    const int HWo = a.Hout * a.Wout;
    // staging roles: this thread owns row mc of the A image and row pc of the B image, parity hA / hB of k,
    // k-pairs [iA0, iA0+A_NI) / [iB0, iB0+B_NI): exactly the values one MFMA lane will read back.
    // A: thread owns 4 consecutive output channels (one float4 per k row) and A_NJ k rows of one parity
    const int mg = t % A_MG;                 // m = mg*4 .. mg*4+3
    const int kqA = t / A_MG;                // 0 .. A_KQ-1
    const int hA = kqA & 1, iA0 = (kqA >> 1) * A_NJ;
    const int pc = t % BN;
    const int gB = __builtin_amdgcn_readfirstlane(t / BN);
    const int hB = gB & 1, iB0 = (gB >> 1) * B_NI;
    const long long p = n0 + pc;
    const bool pvalid = p < a.P;
    int ih0 = 0, iw0 = 0;
    const float* inb = a.in;
    if (pvalid) {
        const int n = (int)(p / HWo);
        const int rem = (int)(p - (long long)n * HWo);
        const int oh = rem / a.Wout, ow = rem - oh * a.Wout;
        ih0 = oh * a.stride - a.pad;
        iw0 = ow * a.stride - a.pad;
        inb = a.in + (size_t)n * a.Cin * a.Hin * a.Win;
        if (ONE) inb += (size_t)ih0 * a.Win + iw0;
    }
    const size_t HWin = (size_t)a.Hin * a.Win;
    const float* wcol = a.wT + m0 + mg * 4;
    // VECB staging role: pixels pg*4 .. pg*4+3 of the tile (same image: HWo % 4 == 0), B_NJ k rows of parity hV
    const int pg = t % B_PG, kqB = t / B_PG;
    const int hV = kqB & 1, iV0 = (kqB >> 1) * B_NJ;
    const float* inv = a.in;
    bool vvalid = false;
    if (VECB) {
        const long long pv4 = n0 + pg * 4;
        vvalid = pv4 < a.P;
        if (vvalid) {
            const int n = (int)(pv4 / HWo);
            inv = a.in + (size_t)n * a.Cin * HWin + (size_t)(pv4 - (long long)n * HWo);  // stride 1, pad 0: same plane offset
        }
    }
    f32x4 rv[B_NJ];

    f32x4 ra[A_NJ];
    float rb[B_NI];
    // Validity of the B-side values of the step in flight, one bit per load.  It is applied when the registers are
    // written to LDS, NOT at the load: a select on a just-loaded value makes the compiler wait for that load on the
    // spot, which serialises the gather on memory latency (and, with the loads pinned ahead of the MFMAs, would stall
    // the whole step).  Invalid elements read a valid dummy address.
    unsigned okmask = 0;

    auto load_global = [&](int k0) {
#pragma unroll
        for (int j = 0; j < A_NJ; ++j)
            ra[j] = *reinterpret_cast<const f32x4*>(wcol + (size_t)(k0 + hA + 2 * (iA0 + j)) * a.Mpad);
        if (VECB) {
            okmask = 0;
#pragma unroll
            for (int j = 0; j < B_NJ; ++j) {
                const int k = k0 + hV + 2 * (iV0 + j);
                const bool ok = vvalid & (k < a.Cin);
                okmask |= ok ? (1u << j) : 0u;
                rv[j] = *reinterpret_cast<const f32x4*>(inv + (size_t)(ok ? k : 0) * HWin);
            }
            return;
        }
        if (ONE) {
            okmask = 0;
#pragma unroll
            for (int i = 0; i < B_NI; ++i) {
                const int k = k0 + hB + 2 * (iB0 + i);
                const bool ok = pvalid & (k < a.Cin);
                okmask |= ok ? (1u << i) : 0u;
                rb[i] = inb[(size_t)(ok ? k : 0) * HWin];
            }
            return;
        }
        // ktab is stored per 32-k block as [16 even k | 16 odd k]: this wave's B_NI entries are contiguous
        // -> one wide scalar load and a single wait instead of a dependent s_load per element
        const int32_t* kt = a.ktab + k0 + hB * KK + iB0;
        int ev[B_NI];
#pragma unroll
        for (int i = 0; i < B_NI; ++i) ev[i] = kt[i];
        okmask = 0;
#pragma unroll
        for (int i = 0; i < B_NI; ++i) {
            const int e = ev[i];
            const int cin = e >> 8, kh = (e >> 4) & 15, kw = e & 15;
            const int ih = ih0 + kh, iw = iw0 + kw;
            // bitwise & (no short-circuit): keeps the gather branch-free (v_cndmask, not exec-mask branches)
            const bool ok = pvalid & (e >= 0) & ((unsigned)ih < (unsigned)a.Hin) & ((unsigned)iw < (unsigned)a.Win);
            const int off = (cin * a.Hin + ih) * a.Win + iw;
            okmask |= ok ? (1u << i) : 0u;
            rb[i] = inb[ok ? off : 0];  // always a valid address; masked in store_lds
        }
    };
    auto store_lds = [&](int buf) {
        const int swb = (pc >> 2) & 3;
        // 4x(A_NJ) register transpose: element (j, e) of the loaded rows is k-pair iA0+j of channel mg*4+e
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = mg * 4 + e;
            float* dst = &As[buf][hA][m][0];
            if (A_NJ == 4) {
                f32x4 v = {ra[0][e], ra[1][e], ra[2][e], ra[3][e]};
                *reinterpret_cast<f32x4*>(dst + (((iA0 >> 2) ^ (mg & 3)) << 2)) = v;   // (m>>2)&3 == mg&3
            } else {
                float2 v;
                v.x = ra[0][e]; v.y = ra[1][e];
                *reinterpret_cast<float2*>(dst + (((iA0 >> 2) ^ (mg & 3)) << 2) + (iA0 & 3)) = v;
            }
        }
        if (VECB) {
#pragma unroll
            for (int j = 0; j < B_NJ; ++j) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                rv[j] = ((okmask >> j) & 1u) ? rv[j] : z;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float* dst = &Bs[buf][hV][pg * 4 + e][0];
                if (B_NJ == 4) {
                    f32x4 v = {rv[0][e], rv[1][e], rv[2][e], rv[3][e]};
                    *reinterpret_cast<f32x4*>(dst + (((iV0 >> 2) ^ (pg & 3)) << 2)) = v;
                } else {
                    float2 v;
                    v.x = rv[0][e]; v.y = rv[1][e];
                    *reinterpret_cast<float2*>(dst + (((iV0 >> 2) ^ (pg & 3)) << 2) + (iV0 & 3)) = v;
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < B_NI; ++i) rb[i] = ((okmask >> i) & 1u) ? rb[i] : 0.0f;
#pragma unroll
        for (int q = 0; q < B_NI / 4; ++q) {
            f32x4 v = {rb[4 * q], rb[4 * q + 1], rb[4 * q + 2], rb[4 * q + 3]};
            *reinterpret_cast<f32x4*>(&Bs[buf][hB][pc][((iB0 / 4 + q) ^ swb) * 4]) = v;
        }
    };

    f32x16 acc[TM][TN];
    acc_zero(acc);

    const int lrow = lane >> 5, lcol = lane & 31;
    auto compute = [&](int cur) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {  // two halves of 8 k-pairs keep the fragment registers at 32
            f32x4 af[TM][2], bf[TN][2];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = (wm * TM + i) * 32 + lcol;
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    af[i][q] = *reinterpret_cast<const f32x4*>(&As[cur][lrow][m][((half * 2 + q) ^ ((m >> 2) & 3)) * 4]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int pl = (wn * TN + j) * 32 + lcol;
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    bf[j][q] = *reinterpret_cast<const f32x4*>(&Bs[cur][lrow][pl][((half * 2 + q) ^ ((pl >> 2) & 3)) * 4]);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][q][e], bf[j][q][e], acc[i][j], 0, 0, 0);
        }
    };

    const int nk = a.Kpad / BK;
    if (WS) {
        if (__builtin_amdgcn_readfirstlane(tid >> 8) != 0) {
            // ---- loader wavefronts: tile kt+1 is written to LDS during step kt, tile kt+2 is in flight ----
            load_global(0);
            store_lds(0);
            if (nk > 1) load_global(BK);
            __syncthreads();
            for (int kt = 0; kt < nk; ++kt) {
                if (kt + 1 < nk) store_lds((kt + 1) & 1);
                if (kt + 2 < nk) load_global((kt + 2) * BK);
                __syncthreads();
            }
            return;
        }
        // ---- MFMA wavefronts ----
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            compute(kt & 1);
            __syncthreads();
        }
    } else {
        load_global(0);
        store_lds(0);
        __syncthreads();
        RFX_STAMP(1);
        int cur = 0;
        for (int kt = 0; kt < nk; ++kt) {
            // branch-free body (the last step re-loads its own tile into the unused buffer): one basic block, so the
            // scheduler is free to interleave the gather of step kt+1 with the MFMAs of step kt
            load_global((kt + 1 < nk ? kt + 1 : kt) * BK);
            __builtin_amdgcn_sched_barrier(0);   // the loads stay AHEAD of the MFMAs: left to itself the scheduler sinks them
            compute(cur);                        // to the end of the step and their latency is exposed at every barrier
            __builtin_amdgcn_sched_barrier(0);   // ... and nothing that consumes them is hoisted into the MFMA stream
            store_lds(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
    }

    RFX_STAMP(2);
    // epilogue (conv_epilogue.h): this lane's pixel of each 32-pixel sub-tile -> plane offset
    size_t pix_off[TN];
    bool pix_ok[TN];
    pix_linear<TN>(pix_off, pix_ok, n0 + wn * TN * 32 + lcol, a.P, HWo, a.Cout);
    conv_epilogue<TM, TN, WS>(acc, s_scale, s_shift, a.res, a.out, a.act, a.Cout, (size_t)HWo, m0, wm, lrow, pix_off, pix_ok,
                              m0 + BM <= a.Cout);
#ifdef RFX_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    RFX_STAMP(3);
#endif
}

template <int TM, int TN, bool ONE, bool WS, bool VECB>
using ConvGemm = RfxFamily<ConvArgs, conv2d_mfma_body<TM, TN, ONE, WS, VECB>, WS ? 512 : 256, WS ? 4 : 2>;

template <int TM, int TN, bool ONE, bool WS, bool VECB>
__global__ __launch_bounds__((ConvGemm<TM, TN, ONE, WS, VECB>::BLOCK), (ConvGemm<TM, TN, ONE, WS, VECB>::min_waves())) void conv2d_mfma_kernel(ConvArgs a) {
    conv2d_mfma_body<TM, TN, ONE, WS, VECB>(a, blockIdx.x, gridDim.x);
}

template <int TM, int TN, bool ONE, bool WS, bool VECB>
static int launch_conv(ConvArgs& a, hipStream_t st) {
    constexpr int BM = 64 * TM, BN = 64 * TN;
    a.tilesM = (a.Cout + BM - 1) / BM;
    a.tilesP = (int)((a.P + BN - 1) / BN);
    const long long nwg = (long long)a.tilesM * a.tilesP;
    if (nwg > 0x7fffffffLL) return RFX_E_LIMIT;
#ifdef RFX_TRACE
    a.trace = g_trace;
#endif
    return ConvGemm<TM, TN, ONE, WS, VECB>::launch(conv2d_mfma_kernel<TM, TN, ONE, WS, VECB>, a, (unsigned)nwg, st);
}

// Every instance of the implicit-GEMM kernel the library builds (conv_dispatch.h decides which one a launch takes): the three tiles
// with and without the 1x1 specialisation, wave-specialised on the two larger tiles, and the three 1x1 tiles with vectorised
// pixel-side loads (never wave-specialised).
struct GemmEntry {
    int key;
    int (*launch)(ConvArgs&, hipStream_t);
};
#define G(TM, TN, ONE, WS, VECB) {ConvInstance::gemm(TM, TN, ONE, WS, VECB).id(), &launch_conv<TM, TN, ONE, WS, VECB>}
static const GemmEntry kGemm[] = {
    G(2, 2, false, false, false), G(2, 2, true, false, false), G(2, 2, false, true, false), G(2, 2, true, true, false),
    G(1, 2, false, false, false), G(1, 2, true, false, false), G(1, 2, false, true, false), G(1, 2, true, true, false),
    G(1, 1, false, false, false), G(1, 1, true, false, false),
    G(2, 2, true, false, true), G(1, 2, true, false, true), G(1, 1, true, false, true),
};
#undef G

extern "C" int rfx_conv2d_tile_variant(int N, int Cout, int Hout, int Wout) {
    return conv_tile_variant(conv_knobs(), N, Cout, Hout, Wout);
}

extern "C" int rfx_conv2d_kernel_id(int N, int Cin, int Cout, int KH, int KW, int stride, int pad, int Hout,
                                    int Wout) {
    return conv_decide(conv_knobs(), {N, Cin, Cout, KH, KW, stride, pad, Hout, Wout}, true, 0, true, rfx_group_recording()).id();
}

// The direct 3x3 kernel with the weights in its own packed order (conv3x3.hip); bit 5 of rfx_conv2d_kernel_id says when
// it applies.  rfx_conv2d_f32 computes the same convolution, bit for bit, from the generic wT / ktab packing.
extern "C" int rfx_conv3x3_f32(const float* in, const float* wP, const float* scale, const float* shift,
                               const float* residual, float* out, int N, int Cin, int H, int W, int Cout, int act,
                               int k_chunk, void* stream) {
    if (!in || !wP || !out || N <= 0 || Cin < 8 || H <= 0 || W <= 0 || Cout <= 0) return RFX_E_ARG;
    if (reinterpret_cast<uintptr_t>(wP) & 15) return RFX_E_ARG;
    if ((long long)Cin * H * W > 0x7fffffffLL) return RFX_E_LIMIT;
    if (k_chunk != 0 && k_chunk != 4) return RFX_E_ARG;                      // the one chunk length the kernels are built for
    return rfx_conv3x3_direct_launch(conv_direct3x3(conv_knobs(), N, Cin, Cout, H, W, k_chunk, rfx_group_recording()), in, wP, scale, shift, residual,
                                     out, N, Cin, H, W, Cout, (Cout + 127) / 128 * 128, act, rfx_stream(stream));
}

extern "C" int rfx_conv3x3_kernel_id(int N, int Cin, int Cout, int H, int W, int k_chunk) {
    return conv_decide(conv_knobs(), {N, Cin, Cout, 3, 3, 1, 1, H, W}, true, k_chunk, true, rfx_group_recording()).id();
}

// The direct stride-2 kernel with the packed weights of rfx_conv3x3_f32 (bit 13 of rfx_conv2d_kernel_id says when it applies).
extern "C" int rfx_conv3x3_s2_f32(const float* in, const float* wP, const float* scale, const float* shift,
                                  const float* residual, float* out, int N, int Cin, int H, int W, int Cout, int act,
                                  void* stream) {
    if (!in || !wP || !out || N <= 0 || Cin < 8 || Cin % 8 != 0 || H <= 0 || W <= 0 || Cout <= 0) return RFX_E_ARG;
    if (reinterpret_cast<uintptr_t>(wP) & 15) return RFX_E_ARG;
    const ConvInstance ci = conv_direct3x3_s2(conv_knobs(), N, Cin, Cout, (H - 1) / 2 + 1, (W - 1) / 2 + 1, rfx_group_recording());
    return rfx_conv3x3_s2_launch(ci, in, wP, scale, shift, residual, out, N, Cin, H, W, Cout, act, rfx_stream(stream));
}

// dil = 1: rfx_conv2d_f32.  dil > 1 (rfx_conv2d_dilated_f32): the gather adds the ktab's (kh, kw) fields to the window origin
// as they are, so a dilated convolution is the SAME kernel with a table that holds kh*dil / kw*dil -- only the output size and the
// 4-bit field limit know about the dilation.
static int conv2d_impl(const float* in, const float* wT, const int32_t* ktab, const float* scale,
                       const float* shift, const float* residual, float* out, int N, int Cin, int Hin,
                       int Win, int Cout, int KH, int KW, int stride, int pad, int dil, int act, void* stream) {
    if (!in || !wT || !ktab || !out) return RFX_E_ARG;
    if (N <= 0 || Cin <= 0 || Hin <= 0 || Win <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0 || dil <= 0)
        return RFX_E_ARG;
    if ((KH - 1) * dil + 1 > 15 || (KW - 1) * dil + 1 > 15 || Cin >= (1 << 22)) return RFX_E_LIMIT;
    ConvArgs a;
    a.in = in; a.wT = wT; a.ktab = ktab; a.scale = scale; a.shift = shift; a.res = residual; a.out = out;
    a.N = N; a.Cin = Cin; a.Hin = Hin; a.Win = Win; a.Cout = Cout; a.stride = stride; a.pad = pad; a.act = act;
    a.Hout = (Hin + 2 * pad - ((KH - 1) * dil + 1)) / stride + 1;
    a.Wout = (Win + 2 * pad - ((KW - 1) * dil + 1)) / stride + 1;
    if (a.Hout <= 0 || a.Wout <= 0) return RFX_E_ARG;
    if ((long long)Cin * Hin * Win > 0x7fffffffLL) return RFX_E_LIMIT;
    const int K = Cin * KH * KW;
    a.Kpad = (K + 31) / 32 * 32;
    a.Mpad = (Cout + 127) / 128 * 128;
    a.P = (long long)N * a.Hout * a.Wout;
    hipStream_t st = rfx_stream(stream);
    const ConvInstance ci = conv_decide(conv_knobs(), {N, Cin, Cout, KH, KW, stride, pad, a.Hout, a.Wout}, false, 0,
                                        (reinterpret_cast<uintptr_t>(in) & 15) == 0, rfx_group_recording());
    if (ci.family == CONV_KMAJOR)
        return rfx_conv1x1_kmajor_launch(ci, in, wT, scale, shift, residual, out, N, Cin, Hin * Win, Cout, a.Mpad, act, st);
    const GemmEntry* e = conv_find(kGemm, ci);
    return e ? e->launch(a, st) : RFX_E_ARG;
}

extern "C" int rfx_conv2d_f32(const float* in, const float* wT, const int32_t* ktab, const float* scale,
                              const float* shift, const float* residual, float* out, int N, int Cin, int Hin,
                              int Win, int Cout, int KH, int KW, int stride, int pad, int act, void* stream) {
    return conv2d_impl(in, wT, ktab, scale, shift, residual, out, N, Cin, Hin, Win, Cout, KH, KW, stride, pad, 1, act, stream);
}

extern "C" int rfx_conv2d_dilated_f32(const float* in, const float* wT, const int32_t* ktab, const float* scale,
                                      const float* shift, const float* residual, float* out, int N, int Cin, int Hin,
                                      int Win, int Cout, int KH, int KW, int stride, int pad, int dilation, int act,
                                      void* stream) {
    if (dilation == 1) return RFX_E_ARG;      // the undilated geometries belong to rfx_conv2d_f32 / rfx_conv3x3_f32
    return conv2d_impl(in, wT, ktab, scale, shift, residual, out, N, Cin, Hin, Win, Cout, KH, KW, stride, pad, dilation, act, stream);
}
