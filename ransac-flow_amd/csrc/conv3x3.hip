// conv3x3.hip -- direct 3x3 / stride 1 / pad 1 convolution on the fp32 MFMA (the heaviest layer class of the path:
// ResNet-50 Bottleneck conv2 at stride 1, model/resnet50.py:75; every BasicBlock conv of the FeatureExtractor,
// model/model.py:32-35; the NetFlowCoarse / NetMatchability stacks, model/model.py:170-181).
//
// The implicit-GEMM kernel of conv.hip gathers its im2col operand element by element: ~10 address / bounds
// instructions per gathered float, which is what holds it at ~60 % of the matrix peak.  Here a workgroup owns an
// 8 x 16 patch of output pixels of ONE image and stages the RAW input patch (10 x 18 per channel, zero filled at the
// image border) in LDS once per 8 input channels; the MFMA B operand for tap (c, kh, kw) of pixel (r, x) is then the
// LDS word [c][r+kh][x+kw] -- fetched with one ds_read_b32 at a per-lane address that is precomputed ONCE (the 36
// k-pair offsets of a K step repeat every step).  No per-element index arithmetic is left in the loop:
//     per K step (72 = 8 channels x 9 taps): 9 float4 weight loads + 6 input loads per thread,
//     then per wavefront 18 ds_read_b128 (A) + 72 ds_read_b32 (B) + 144 MFMAs.
// A operand (weights): LDS image [k&1][m][k>>1] with 36 k-pairs per row (row stride 144 B: the 16-lane ds_read_b128
// groups hit 16 distinct bank quads without a swizzle because 9 is odd).  The host packs the weights ONCE in exactly
// that order (rfx_api.h: "wP"), one contiguous 36 KB image per (128-channel tile, K step), so staging is a straight
// 16-byte-per-lane copy: coalesced global loads, conflict-free ds_write_b128, no register transposes.
// The global loads of step s+1 are not issued as one burst: they are dealt out two at a time between the 16-MFMA
// chunks of step s, where they issue in the shadow of the matrix pipe (a burst in front of the MFMAs cost 13 % of
// the kernel, the bank-conflicting transposed stores another 8 %: scripts/ubench/conv_bench.py).
// B patch rows are 48 floats apart so that the two 16-pixel rows a 32-lane half reads fall on disjoint banks.
// Numerics: k runs channel-major, taps row-major -- the same order as conv.hip / the packed weight matrix, so the
// result is bit-identical to the implicit-GEMM kernel.
#include "common.h"
#include "conv_dispatch.h"
#include "conv_epilogue.h"
#include "conv_tile.h"
#include "group.h"

namespace {

// Output patch of a workgroup: 128 pixels as PT_R x PT_C = 8x16, 16x8 or 32x4 (the host picks the shape that wastes
// the fewest pixels on the image at hand: the trunk runs on 25x33 ... 36x48 maps at its small scales).  A 32-lane half
// of a B read covers 32/PT_C patch rows; the LDS row stride BS puts those rows on disjoint banks:
//   PT_C 16 -> 2 rows,  BS 48 (row offsets 0,16);  PT_C 8 -> 4 rows, BS 24 (0,24,16,8);  PT_C 4 -> 8 rows, BS 12 (0,12,24,4,16,28,8,20).
// The images of a batch are tiled as ONE tall map: image n occupies rows n*(H+1) .. n*(H+1)+H-1 of a stack whose row
// n*(H+1)+H is a virtual all-zero row -- at once the bottom halo of image n and the top halo of image n+1.  Patches tile
// the stack, so a patch may straddle two (or, on tiny maps, several) images and only the LAST patch row of the whole batch
// is ragged: a 25x33 map costs 26/25 instead of 32/25 in the row direction (the 7-level pyramid puts a quarter of the
// 3x3 work on such maps).  Outputs that fall on a virtual row are computed and dropped (1/(H+1) of the work).
// TN = 32-pixel MFMA sub-tiles per wavefront: 2 -> 128 pixels per workgroup; 4 -> 256 pixels (16 x 16 patch) for the layers
// whose output channels all fit one 64-channel tile (TM = 1): there the 18 KB weight image of a K step dwarfs the 6 KB input
// patch, and twice the pixels per workgroup halve the weight bytes a CU pulls per MFMA (the 64-channel layers sit on the CU's
// load path).  Same k order per output element: bit-identical to TN = 2.
template <int PT_C_, int TN_ = 2> struct Patch {
    static constexpr int PT_C = PT_C_, PT_R = 64 * TN_ / PT_C_;
    static constexpr int PR = PT_R + 2, PC = PT_C + 2;        // input patch incl. halo
    static constexpr int BS = PT_C_ == 16 ? 48 : (PT_C_ == 8 ? 24 : 12);
    static constexpr int RH = 32 / PT_C_;                     // patch rows per 32-pixel MFMA sub-tile
};
constexpr int CH = 8;                        // input channels per K step
constexpr int KS = CH * 9;                   // 72 k per step
constexpr int KK = KS / 2;                   // 36 k-pairs

struct C3Args {
    const float* in; const float* wT;   // wT: the packed image wP (rfx_api.h)
    const float* scale; const float* shift; const float* res; float* out;
    int N, Cin, H, W, Cout, act, Mpad;
    int tilesM, tilesH, tilesW;
    // FUSE: the 1x1 expansion that follows (Bottleneck conv3 + bn3 + residual + ReLU, model/resnet50.py:77-79,99-103)
    const float* wT3; const float* scale3; const float* shift3;
    int Cexp, Mpad3, act3;
#ifdef RFX_TRACE
    long long* trace;
#endif
};
#ifdef RFX_TRACE
#define RFX_STAMP(i) do { if (threadIdx.x == 0 && a.trace) a.trace[(size_t)blockIdx.x * 4 + (i)] = wall_clock64(); } while (0)
extern "C" long long* rfx_debug_trace_ptr();
#else
#define RFX_STAMP(i)
#endif

// Staging roles of the packed weights wP (rfx_api.h): the image of a (128-channel tile, K step) is two parity planes of 128 rows x 36
// k-pairs; a workgroup's share is A_F4 consecutive float4 (TM = 2: the whole 36 KB image; TM = 1: the rows of its 64-channel half
// inside both planes); thread t copies float4 t, t + 256, ... (TM = 1: the 128 surplus slots of the last round re-copy float4
// 0..127 -- same value to the same place).  The bodies keep the per-thread tables; the helpers return one entry (filling the
// tables through array references costs the 32x4-patch instances a register or two).
template <int TM>
struct WpStage {
    static constexpr int A_F4 = 2 * 64 * TM * KK / 4, NA = (A_F4 + 255) / 256;     // 2304 / 1152 float4, 9 / 5 per thread
    static constexpr int PLANE_B = 128 * KK * 4;                                    // bytes of one parity plane of a packed image
    static constexpr size_t STEP_B = (size_t)2 * PLANE_B;                           // bytes per (tile, step)
    static __device__ __forceinline__ int lds_f4(int t, int j) {          // float4 index inside As of thread t's j-th copy
        const int L = t + 256 * j;
        return L >= A_F4 ? L - A_F4 : L;
    }
    static __device__ __forceinline__ unsigned src_off(int L) {           // its byte offset inside the packed image of a step
        return TM == 2 ? (unsigned)(L * 16) : (unsigned)((L / (A_F4 / 2)) * PLANE_B + (L % (A_F4 / 2)) * 16);
    }
    static __device__ __forceinline__ const char* tile(const float* wP, int m0, int nsteps) {      // this tile's image of step 0
        return reinterpret_cast<const char*>(wP) + (size_t)(m0 / 128) * nsteps * STEP_B + (TM == 1 ? ((m0 >> 6) & 1) * (PLANE_B / 2) : 0);
    }
};

// FUSE = true: the workgroup's tile holds ALL channels of the 3x3 convolution (Cout == 64*TM); instead of going to HBM
// the tile (after bn + ReLU) becomes, in LDS, the B operand of the 1x1 expansion that follows it in a Bottleneck, and
// the workgroup writes relu(bn3(conv3(.)) + residual) for its 128 pixels and all Cexp channels.  The 64/128-channel
// intermediate never touches HBM, the expansion's launch, prologue and B-operand staging disappear, and its residual /
// output traffic overlaps the MFMA-bound 3x3 main loops of the neighbouring workgroups.  k order and pairing of the
// expansion are those of conv.hip: bit-identical to the two separate kernels.
// KCH > 0 (round 4): CHUNKED ACCUMULATION.  The fp32 MFMA adds a layer's K = 9 Cin products to ONE accumulator in k order; for
// K = 2304 / 4608 (ResNet-50 layer3 conv2, model/resnet50.py:75; NetFlowCoarse / NetMatchability conv2, model/model.py:172) that
// single chain carries 2.3x the round-off of the CPU reference's K-blocked sums (MKL / oneDNN register blocks of a few hundred
// k; profiles/r04_feature_error_*.json, r04_summation_order_model.json) -- the reason the device's arg-max near-ties flip more
// often than the reference's flip against itself.  With KCH the accumulators are added to a second set every KCH K steps
// (KCH * 72 k) and restarted from zero: total = ((c1 + c2) + c3) + ..., the same blocked sum.  The 64 extra registers come from
// the per-lane B-address table: baddr[kk] = pixb + (lrow ? c1[kk] : c0[kk]) with compile-time c0 / c1, i.e. ONE v_mad per
// k-pair (lrow * (c1 - c0) + pixb) and c0 as the immediate offset of the ds_read -- 36 VALU per K step instead of 36 registers.
// Dispatch (rfx_conv3x3_chunk_steps): every layer with K >= 2048, and -- round 5 -- the 3x3 convolution of a Bottleneck tail
// (model/resnet50.py:75 in layer1 / layer2: K = 576 / 1152), fused or not: the caller's k_chunk argument (rfx_conv3x3_f32) asks
// for the same chunks in the stand-alone kernel, so the fused tail stays bit-identical to its two-kernel form.
template <int TM, int PTC, bool FUSE, int TN = 2, bool RAG = false, int KCH = 0>
__device__ __forceinline__ void conv3x3_direct_body(const C3Args& a, const unsigned bx, const unsigned) {
    using G = Patch<PTC, TN>;
    static_assert(KCH == 0 || !RAG, "chunked accumulation: Cin % 8 == 0 instances only");
    // the 36-entry table of B offsets stays in registers where 2 x (TM * TN) accumulator tiles leave room for it (64-channel
    // tiles of 128 pixels: 32 + 32 accumulators); the other chunked instances recompute an offset per use (one v_mad)
    constexpr bool BTAB = KCH == 0 || TM * TN <= 2;
    static_assert(TN == 2 || (TN == 4 && TM == 1 && PTC == 16), "the 256-pixel patch is built for 64-channel tiles, 16 x 16");
    constexpr int NPX = 64 * TN;                     // output pixels of the workgroup
    constexpr int PT_R = G::PT_R, PT_C = G::PT_C, PR = G::PR, PC = G::PC, BS = G::BS, RH = G::RH;
    constexpr int NB = (CH * PR * PC + 255) / 256;   // patch elements per thread (6; 7 for the 32x4 patch)
    static_assert(PC < BS, "the surplus staging slots live in the never-read padding columns");
    constexpr int BM = 64 * TM;
    constexpr int AS_F = 2 * BM * KK, BS_F = CH * PR * BS, T2_F = FUSE ? BM * NPX : 0;
    constexpr int SMEM_F = AS_F + BS_F > T2_F ? AS_F + BS_F : T2_F;
    __shared__ __attribute__((aligned(16))) float smem[SMEM_F];   // FUSE: the main-loop buffers are reused for the mid tile
    float (*As)[BM][KK] = reinterpret_cast<float (*)[BM][KK]>(smem);
    float (*Bs)[PR][BS] = reinterpret_cast<float (*)[PR][BS]>(smem + AS_F);
    __shared__ float s_scale[BM], s_shift[BM];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = lane >> 5, lcol = lane & 31;

    RFX_STAMP(0);
    // m-tile fastest: the workgroups sharing one input patch sit on one L2 (tilesH counts patch rows of the whole stack)
    const int bid = xcd_remap(bx, a.tilesM * a.tilesH * a.tilesW);
    const int m0 = (bid % a.tilesM) * BM;
    const int pt = bid / a.tilesM;
    const int R0 = (pt / a.tilesW) * PT_R, ow0 = (pt % a.tilesW) * PT_C;    // first stack row / column of the patch
    const int Hs = a.H + 1, Rtot = a.N * Hs;                                 // stack period, stack height
    const size_t HW = (size_t)a.H * a.W;
    const int nbase = (R0 > 0 ? R0 - 1 : 0) / Hs;                            // image of the first input row of the patch
    const float* inn = a.in + (size_t)nbase * a.Cin * HW;                    // 32-bit patch offsets are relative to it

    stage_bn<BM>(s_scale, s_shift, a.scale, a.shift, m0, a.Cout);

    // ---- staging roles ----
    constexpr int NA = WpStage<TM>::NA;
    constexpr size_t step_b = WpStage<TM>::STEP_B;
    unsigned aoff[NA];    // byte offset inside the packed image of a step
    int alds[NA];         // float4 index inside As
#pragma unroll
    for (int j = 0; j < NA; ++j) { alds[j] = WpStage<TM>::lds_f4(t, j); aoff[j] = WpStage<TM>::src_off(alds[j]); }
    // Cin need not be a multiple of CH (the 49-channel correlation volume in front of the heads, model/model.py:213): the
    // packed weights carry zero rows for the missing channels of the last K step, and the patch slots of those channels are
    // zero filled (their loads point at the first channel of the step: a valid address) -- the sum gains exact zeros only.
    const int nsteps = (a.Cin + CH - 1) / CH;
    const int crem = a.Cin - (nsteps - 1) * CH;                        // channels of the last K step
    const bool ragged = RAG && crem != CH;                             // RAG: its own kernel instance (the host picks it when Cin % 8 != 0)
    const char* wtile = WpStage<TM>::tile(a.wT, m0, nsteps);
    // input patch: NB of the CH*PR*PC (1440 or 1632) patch elements per thread (the surplus slots land in the unused
    // columns of the last patch row, so that every load is consumed unconditionally: no divergent store).
    unsigned boffB[NB];   // byte offset inside one channel group (cl*HW + gy*W + gx)*4; 0 with bok=false -> zero
    bool bok[NB];
    unsigned clok = 0;    // bit u: the channel of slot u exists in the LAST K step
    int blds[NB];        // LDS float index
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int idx = t + 256 * u;
        const bool real = idx < CH * PR * PC;
        const int cl = idx / (PR * PC), rem = idx - cl * (PR * PC);
        const int pr = rem / PC, px = rem - pr * PC;
        const int Rin = R0 - 1 + pr, gx = ow0 - 1 + px;                      // stack row -> (image, row); row H is virtual
        const int ni = (Rin >= 0 ? Rin : 0) / Hs, gy = Rin - ni * Hs;
        bok[u] = real && Rin >= 0 && Rin < Rtot && gy < a.H && (unsigned)gx < (unsigned)a.W;
        clok |= (cl < crem) ? (1u << u) : 0u;
        boffB[u] = bok[u] ? ((unsigned)((ni - nbase) * a.Cin + cl) * (unsigned)HW + (unsigned)(gy * a.W + gx)) * 4u : 0u;
        blds[u] = real ? (cl * PR + pr) * BS + px : ((CH - 1) * PR + PR - 1) * BS + PC + (idx - CH * PR * PC) % (BS - PC);
    }

    f32x4 ra[NA];
    float rb[NB];
    constexpr int NLD = NB + NA;                 // global loads per thread and step: patch first, then weights
    constexpr int LPC = 2;                       // ... dealt out LPC per 16-MFMA chunk
    static_assert(LPC * 8 >= NLD, "all loads of a step are issued before its last chunk");
    // `last` (wave-uniform): the tile is the ragged last K step -- slots of channels >= Cin load from offset 0 and store zeros
    auto load_one = [&](int id, const char* wstep, const char* base, bool last) {
        if (id < NB) rb[id] = *reinterpret_cast<const float*>(base + ((last && !((clok >> id) & 1u)) ? 0u : boffB[id]));   // masked at store time
        else if (id < NLD) ra[id - NB] = *reinterpret_cast<const f32x4*>(wstep + aoff[id - NB]);
    };
    auto load_global = [&](int s, bool last) {
        const char* wstep = wtile + (size_t)s * step_b;
        const char* base = reinterpret_cast<const char*>(inn + (size_t)s * CH * HW);
#pragma unroll
        for (int id = 0; id < NLD; ++id) load_one(id, wstep, base, last);
    };
    auto store_lds = [&](bool last) {
        f32x4* a4 = reinterpret_cast<f32x4*>(smem);
#pragma unroll
        for (int j = 0; j < NA; ++j) a4[alds[j]] = ra[j];
        float* bflat = &Bs[0][0][0];
#pragma unroll
        for (int u = 0; u < NB; ++u) bflat[blds[u]] = (bok[u] && (!last || ((clok >> u) & 1u))) ? rb[u] : 0.0f;
    };

    // ---- per-lane B addresses of the 36 k-pairs of a step (identical for every step) ----
    const int pixb = (wn * TN * RH + lcol / PT_C) * BS + lcol % PT_C;   // sub-tile j adds RH rows = RH*BS
    // patch offset of tap k = c*9 + kh*3 + kw (compile-time for a constant k)
    auto koff = [](int k) constexpr { return (k / 9) * (PR * BS) + ((k % 9) / 3) * BS + (k % 9) % 3; };
    int baddr[BTAB ? KK : 1];
    if constexpr (BTAB) {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) baddr[kk] = pixb + (lrow ? koff(2 * kk + 1) : koff(2 * kk));
    }
    int pixb_cur = pixb;               // !BTAB: laundered once per K step so that the 36 step-invariant indices are NOT hoisted
    auto b_index = [&](int kk) {       // !BTAB: recomputed per use (one v_mad); else the table
        if constexpr (BTAB) return baddr[kk];
        else return pixb_cur + koff(2 * kk) + lrow * (koff(2 * kk + 1) - koff(2 * kk));
    };

    f32x16 acc[TM][TN];
    acc_zero(acc);

    f32x16 tot[KCH ? TM : 1][KCH ? TN : 1];
    if constexpr (KCH > 0) acc_zero(tot);
    load_global(0, ragged && nsteps == 1);
    store_lds(ragged && nsteps == 1);
    __syncthreads();
    RFX_STAMP(1);
    const float* bflat = &Bs[0][0][0];
    for (int s = 0; s < nsteps; ++s) {
        const int sn = s + 1 < nsteps ? s + 1 : s;     // the last step re-loads its own tile: harmless
        const bool lastn = ragged && sn == nsteps - 1;
        const char* wstep = wtile + (size_t)sn * step_b;
        const char* base = reinterpret_cast<const char*>(inn + (size_t)sn * CH * HW);
        // LDS reads run one 4-k-pair chunk ahead of the MFMAs that consume them (register double buffer)
        f32x4 af[2][TM];
        float bv[2][4 * TN];
        if constexpr (!BTAB) { pixb_cur = pixb; asm volatile("" : "+v"(pixb_cur)); }
        auto read_chunk = [&](int q, int slot) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[slot][i] = *reinterpret_cast<const f32x4*>(&As[lrow][(wm * TM + i) * 32 + lcol][q * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int j = 0; j < TN; ++j) bv[slot][TN * e + j] = bflat[b_index(q * 4 + e) + j * RH * BS];
            }
        };
        read_chunk(0, 0);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const int cur = q & 1;
            if (q + 1 < 9) read_chunk(q + 1, cur ^ 1);
#pragma unroll
            for (int i = 0; i < LPC; ++i) load_one(q * LPC + i, wstep, base, lastn);   // tile s+1, in the MFMA shadow
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i][e], bv[cur][TN * e + j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (KCH > 0) {
            if ((s + 1) % KCH == 0 || s + 1 == nsteps) acc_close_chunk(tot, acc);      // wave-uniform
        }
        __syncthreads();   // everyone is done reading the tile
        store_lds(lastn);   // tile s+1
        __syncthreads();
    }

    RFX_STAMP(2);
    // ---- epilogue (conv_epilogue.h) ----
    const int Cfinal = FUSE ? a.Cexp : a.Cout;
    // element offset / existence of this lane's pixel in MFMA sub-tile st (32 consecutive pixels = RH patch rows) of the patch
    auto pixel_of = [&](int st, size_t& off, bool& ok) {
        const int R = R0 + st * RH + lcol / PT_C, ow = ow0 + lcol % PT_C;
        const int n = R / Hs, oh = R - n * Hs;
        ok = R < Rtot && oh < a.H && ow < a.W;
        off = ok ? (size_t)n * Cfinal * HW + (size_t)oh * a.W + ow : 0;
    };
    if constexpr (!FUSE) {
        size_t pix_off[TN];
        bool pix_ok[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) pixel_of(wn * TN + j, pix_off[j], pix_ok[j]);
        const bool full = m0 + BM <= a.Cout;
        if constexpr (KCH > 0)
            conv_epilogue<TM, TN, (TM > 1)>(tot, s_scale, s_shift, a.res, a.out, a.act, a.Cout, HW, m0, wm, lrow, pix_off, pix_ok, full);
        else
            conv_epilogue<TM, TN, (TM > 1)>(acc, s_scale, s_shift, a.res, a.out, a.act, a.Cout, HW, m0, wm, lrow, pix_off, pix_ok, full);
    } else {
        // ---- mid tile -> LDS: T2[channel][pixel], pixel = MFMA column numbering (wn*2 + j)*32 + lcol
        float* T2 = smem;   // every wavefront is past the last barrier of the main loop: As / Bs are free
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
                    float v;
                    if constexpr (KCH > 0) v = fmaf(tot[i][j][r], s_scale[ch], s_shift[ch]);
                    else v = fmaf(acc[i][j][r], s_scale[ch], s_shift[ch]);
                    if (a.act == RFX_ACT_RELU) v = v > 0.0f ? v : 0.0f;
                    T2[ch * NPX + (wn * TN + j) * 32 + lcol] = v;
                }
        __syncthreads();
        // ---- 1x1 expansion: out[Cexp x 128 px] = W3[Cexp x BM] * T2, 128 output channels per pass, waves 2 x 2.
        // The weights come in "quad" order wQ[q][lrow][m][4] = W3[m][8q + 2j + lrow] (j = 0..3): the four A operands a lane
        // needs for k-pairs 4q..4q+3 are ONE 16-byte load, and consecutive lanes (channels) read consecutive 16 bytes.
        // (a 256-pixel patch runs the expansion over its two 128-pixel halves one after the other: sub-tiles ph*4 + wn*2 + j)
        constexpr int NQ = BM / 8, AHEAD = 2;
#pragma unroll 1
        for (int ph = 0; ph < TN / 2; ++ph) {
        size_t pix_off[2];
        bool pix_ok[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) pixel_of(ph * 4 + wn * 2 + j, pix_off[j], pix_ok[j]);
        const float* t2col = T2 + lrow * NPX + ph * 128 + wn * 64 + lcol;    // + 2kk*NPX (+ 32 for the second sub-tile)
        // one pass: K loop over the mid tile
        auto run_pass = [&](int mp, f32x16 (&acc2)[2][2]) {
            const f32x4* wq0 = reinterpret_cast<const f32x4*>(a.wT3) + (size_t)lrow * a.Cexp + mp + wm * 64 + lcol;   // + q*2*Cexp (+ 32)
            acc_zero(acc2);
            // L2 -> registers, two quads (8 k-pairs = 32 MFMAs) ahead of use
            // (measured, round 3, profiles/r03_fused_tail_expansion_experiment.jsonl + r03_fused_tail_late_prefetch.jsonl: 4 quads
            // ahead +-0; the pass's residual values fetched in front of this loop -6 % (vmcnt retires in order: the loop's weight
            // waits then wait for the residuals too); fetched inside the loop behind its last weight load -3 % on the 64-channel
            // tail, +1 % on the 128-channel one.  The epilogue's cost is not the latency of its residual loads.)
            f32x4 wq[AHEAD + 1][2];
            auto load_w = [&](int q, int slot) {
                wq[slot][0] = wq0[(size_t)q * 2 * a.Cexp];
                wq[slot][1] = wq0[(size_t)q * 2 * a.Cexp + 32];
            };
            // mid-tile operands from LDS run one quad ahead of the MFMAs as well (register double buffer)
            float bq[2][4][2];
            auto read_b = [&](int q, int slot) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bq[slot][e][0] = t2col[2 * (q * 4 + e) * NPX];
                    bq[slot][e][1] = t2col[2 * (q * 4 + e) * NPX + 32];
                }
            };
#pragma unroll
            for (int q = 0; q < AHEAD && q < NQ; ++q) load_w(q, q);
            read_b(0, 0);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (q + AHEAD < NQ) load_w(q + AHEAD, (q + AHEAD) % (AHEAD + 1));
                if (q + 1 < NQ) read_b(q + 1, (q + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float b0 = bq[q & 1][e][0], b1 = bq[q & 1][e][1];
                    const float w0 = wq[q % (AHEAD + 1)][0][e], w1 = wq[q % (AHEAD + 1)][1][e];
                    acc2[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, b0, acc2[0][0], 0, 0, 0);
                    acc2[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, b1, acc2[0][1], 0, 0, 0);
                    acc2[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, b0, acc2[1][0], 0, 0, 0);
                    acc2[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, b1, acc2[1][1], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        for (int mp = 0; mp < a.Cexp; mp += 128) {
            f32x16 acc2[2][2];
            run_pass(mp, acc2);
            // scale3 / shift3 are read straight from global memory (L1 hits): conv_epilogue only indexes the pointers
            conv_epilogue<2, 2, false>(acc2, a.scale3 + mp, a.shift3 + mp, a.res, a.out, a.act3, a.Cexp, HW, mp, wm, lrow, pix_off,
                                       pix_ok, true);
        }
        }   // pixel halves
    }
#ifdef RFX_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    RFX_STAMP(3);
#endif
}

// (three workgroups per CU for the 64-channel fused tail -- 168 VGPRs, 4 spilled -- measured -2.4 %: profiles/r03_fused_tail_3wgs.jsonl)
template <int TM, int PTC, bool FUSE = false, int TN = 2, bool RAG = false, int KCH = 0>
using Direct3 = RfxFamily<C3Args, conv3x3_direct_body<TM, PTC, FUSE, TN, RAG, KCH>, 256, 2>;

template <int TM, int PTC, bool FUSE = false, int TN = 2, bool RAG = false, int KCH = 0>
__global__ __launch_bounds__((Direct3<TM, PTC, FUSE, TN, RAG, KCH>::BLOCK), (Direct3<TM, PTC, FUSE, TN, RAG, KCH>::min_waves())) void conv3x3_direct_kernel(C3Args a) {
    conv3x3_direct_body<TM, PTC, FUSE, TN, RAG, KCH>(a, blockIdx.x, gridDim.x);
}

// ======================================================================================================================
// Round 4: the direct form for 3x3 / STRIDE 2 / pad 1 (ResNet-50 layer2.0 / layer3.0 conv2, model/resnet50.py:75; the first
// convolution of FeatureExtractor layer2 / layer3, model/model.py:86-95) -- 10 % of the config-3 step on the implicit-GEMM
// kernel at 95 TFLOP/s.  Same scheme as above: a workgroup owns an 8 x 16 patch of OUTPUT pixels of one image and stages the
// raw 17 x 33 input patch of 8 channels per K step; the stride-2 taps of 16 consecutive output pixels would hit every second
// LDS word (2-way bank conflicts), so a patch row is stored de-interleaved, [even columns 0..16 | odd columns at +20], 40 floats
// per row: tap (kh, kw) of output pixel (r, x) is the word (2r + kh) * 40 + (kw & 1) * 20 + x + (kw >> 1) -- consecutive
// pixels read consecutive words, and the two patch rows of a 32-lane half lie 80 words = 16 banks apart.  Weights: the same
// packed images wP as the stride-1 kernel (rfx_api.h), same k order as conv.hip -> bit-identical results.  Images are tiled
// one by one (the stacked-batch trick above needs stride 1).  Cin % 8 == 0.
namespace s2 {
constexpr int PT_R = 8, PT_C = 16, PRI = 2 * PT_R + 1, PCI = 2 * PT_C + 1, PH = 20, BS2 = 40, RH = 2;
constexpr int NEL = CH * PRI * PCI;                  // 4488 input elements per K step
constexpr int NB = (NEL + 255) / 256;                // 18 per thread (the last round is partial)
}  // namespace s2

// KCH > 0 (round 5): chunked accumulation as in conv3x3_direct_body -- ResNet-50 layer2.0 / layer3.0 conv2 (K = 1152 / 2304) and the
// FeatureExtractor's 128 -> 256 strided convolution were the last long-K 3x3 layers summed as ONE fma chain.  The B-offset table is
// recomputed per use there (one v_mad per k-pair) to make room for the second accumulator set.
template <int TM, int KCH = 0>
__device__ __forceinline__ void conv3x3_s2_body(const C3Args& a, const unsigned bx, const unsigned) {
    using namespace s2;
    constexpr int TN = 2, BM = 64 * TM;
    constexpr int AS_F = 2 * BM * KK, BS_F = CH * PRI * BS2;
    __shared__ __attribute__((aligned(16))) float smem[AS_F + BS_F];
    float (*As)[BM][KK] = reinterpret_cast<float (*)[BM][KK]>(smem);
    float* bflat = smem + AS_F;                       // [CH][PRI][BS2]
    __shared__ float s_scale[BM], s_shift[BM];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = lane >> 5, lcol = lane & 31;
    const int Ho = (a.H - 1) / 2 + 1, Wo = (a.W - 1) / 2 + 1;
    const int tilesP = a.tilesH * a.tilesW;           // patches per image
    const int bid = xcd_remap(bx, a.tilesM * tilesP * a.N);      // m-tile fastest
    const int m0 = (bid % a.tilesM) * BM;
    int pt = bid / a.tilesM;
    const int n = pt / tilesP;
    pt -= n * tilesP;
    const int oh0 = (pt / a.tilesW) * PT_R, ow0 = (pt % a.tilesW) * PT_C;
    const size_t HW = (size_t)a.H * a.W, HWo = (size_t)Ho * Wo;
    const float* inn = a.in + (size_t)n * a.Cin * HW;

    stage_bn<BM>(s_scale, s_shift, a.scale, a.shift, m0, a.Cout);
    // ---- staging roles
    constexpr int NA = WpStage<TM>::NA;
    constexpr size_t step_b = WpStage<TM>::STEP_B;
    unsigned aoff[NA];    // byte offset inside the packed image of a step
    int alds[NA];         // float4 index inside As
#pragma unroll
    for (int j = 0; j < NA; ++j) { alds[j] = WpStage<TM>::lds_f4(t, j); aoff[j] = WpStage<TM>::src_off(alds[j]); }
    const int nsteps = a.Cin / CH;
    const char* wtile = WpStage<TM>::tile(a.wT, m0, nsteps);
    // input patch = 136 rows (R = channel * 17 + patch row) x 33 columns per K step.  Thread t stages column px = t & 31 of
    // the rows R = (t >> 5) + 8 u, u = 0..16 (8 x 17 = 136 exactly) and, for t < 136, column 32 of row t -- 18 loads, and NO
    // per-element address tables: the LDS word of (R, px) is R * BS2 + f(px), affine in u (an immediate of the store), and the
    // global offset is base + u * 8 W + cl(u) * (HW - 17 W) with cl(u) = c0(u) + [rg >= th(u)], c0 / th compile-time constants
    // (the tables cost 36 registers and made the 128-channel instance spill).
    const int rg = t >> 5, px = t & 31;
    const int gx = 2 * ow0 - 1 + px, gy0 = 2 * oh0 - 1;
    const bool xok = (unsigned)gx < (unsigned)a.W;
    const unsigned D4 = (unsigned)(HW - (size_t)PRI * a.W) * 4u;            // channel step minus 17 rows, bytes
    const unsigned W4 = (unsigned)a.W * 4u;
    // base of row R = rg (channel 0, patch row rg): may point outside the image (masked by bokm); keep it inside the tensor
    const unsigned base_b = (unsigned)((gy0 + rg) * a.W + gx) * 4u;
    unsigned bokm = 0, clsel = 0;
    constexpr int NBR = 17;
#pragma unroll
    for (int u = 0; u < NBR; ++u) {
        const int R = rg + 8 * u, cl = R / PRI, pr = R - cl * PRI;
        const int gy = gy0 + pr;
        bokm |= (xok && (unsigned)gy < (unsigned)a.H) ? (1u << u) : 0u;
        clsel |= (cl != (8 * u) / PRI) ? (1u << u) : 0u;                      // cl(u) = c0(u) + 1 for this thread's rg
    }
    const int blds0 = rg * BS2 + (px & 1) * PH + (px >> 1);                  // + u * 8 * BS2
    // column 32 (t < 136): row R = t
    const bool has33 = t < CH * PRI;
    const int cl33 = (has33 ? t : 0) / PRI, pr33 = (has33 ? t : 0) - cl33 * PRI;
    const int gx33 = 2 * ow0 - 1 + 32, gy33 = gy0 + pr33;
    const bool ok33 = has33 && (unsigned)gx33 < (unsigned)a.W && (unsigned)gy33 < (unsigned)a.H;
    const unsigned boff33 = ok33 ? ((unsigned)cl33 * (unsigned)HW + (unsigned)(gy33 * a.W + gx33)) * 4u : 0u;
    const int blds33 = (has33 ? t : 0) * BS2 + 16;                           // even column 32 -> slot 16
    f32x4 ra[NA];
    float rb[NB];
    constexpr int NLD = NB + NA;
    constexpr int LPC = 3;
    static_assert(NB == NBR + 1, "17 regular rows + the 33rd column");
    static_assert(LPC * 9 >= NLD, "all loads of a step are issued inside its 9 chunks");
    auto load_one = [&](int id, const char* wstep, const char* base) {
        if (id < NBR) {
            const bool ok = (bokm >> id) & 1u;
            // byte offset relative to the channel group's plane 0 (mod 2^32: a valid element's offset is non-negative and below
            // 4 GB, checked at launch); invalid elements read offset 0 (masked at store time).  The empty asm keeps the compiler
            // from hoisting the 17 step-invariant offsets out of the K loop into registers -- the point of having no tables.
            unsigned bo = base_b;
            asm volatile("" : "+v"(bo));
            const unsigned off = bo + (unsigned)id * 8u * W4 + (unsigned)((8 * id) / PRI) * D4 + (((clsel >> id) & 1u) ? D4 : 0u);
            rb[id] = *reinterpret_cast<const float*>(base + (ok ? off : 0u));
        } else if (id == NBR) {
            rb[id] = *reinterpret_cast<const float*>(base + boff33);
        } else if (id < NLD) {
            ra[id - NB] = *reinterpret_cast<const f32x4*>(wstep + aoff[id - NB]);
        }
    };
    auto store_lds = [&]() {
        f32x4* a4 = reinterpret_cast<f32x4*>(smem);
#pragma unroll
        for (int j = 0; j < NA; ++j) a4[alds[j]] = ra[j];
#pragma unroll
        for (int u = 0; u < NBR; ++u) bflat[blds0 + u * 8 * BS2] = ((bokm >> u) & 1u) ? rb[u] : 0.0f;
        if (has33) bflat[blds33] = ok33 ? rb[NBR] : 0.0f;
    };
    // ---- per-lane B addresses of the 36 k-pairs of a step
    const int pixb = (2 * (wn * TN * RH + lcol / PT_C)) * BS2 + lcol % PT_C;            // sub-tile j adds 2*RH rows of the patch
    auto koff2 = [](int k) constexpr { return (k / 9) * (PRI * BS2) + ((k % 9) / 3) * BS2 + (((k % 9) % 3) & 1) * PH + (((k % 9) % 3) >> 1); };
    constexpr bool BTAB = KCH == 0 || TM == 1;
    int baddr[BTAB ? KK : 1];
    if constexpr (BTAB) {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) baddr[kk] = pixb + (lrow ? koff2(2 * kk + 1) : koff2(2 * kk));
    }
    int pixb_cur = pixb;
    auto b_index = [&](int kk) {
        if constexpr (BTAB) return baddr[kk];
        else return pixb_cur + koff2(2 * kk) + lrow * (koff2(2 * kk + 1) - koff2(2 * kk));
    };
    f32x16 acc[TM][TN];
    acc_zero(acc);
    f32x16 tot[KCH ? TM : 1][KCH ? TN : 1];
    if constexpr (KCH > 0) acc_zero(tot);
    {
        const char* base = reinterpret_cast<const char*>(inn);
#pragma unroll
        for (int id = 0; id < NLD; ++id) load_one(id, wtile, base);
    }
    store_lds();
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int sn = s + 1 < nsteps ? s + 1 : s;
        const char* wstep = wtile + (size_t)sn * step_b;
        const char* base = reinterpret_cast<const char*>(inn + (size_t)sn * CH * HW);
        f32x4 af[2][TM];
        float bv[2][4 * TN];
        if constexpr (!BTAB) { pixb_cur = pixb; asm volatile("" : "+v"(pixb_cur)); }
        auto read_chunk = [&](int q, int slot) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[slot][i] = *reinterpret_cast<const f32x4*>(&As[lrow][(wm * TM + i) * 32 + lcol][q * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < TN; ++j) bv[slot][TN * e + j] = bflat[b_index(q * 4 + e) + j * 2 * RH * BS2];
        };
        read_chunk(0, 0);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const int cur = q & 1;
            if (q + 1 < 9) read_chunk(q + 1, cur ^ 1);
#pragma unroll
            for (int i = 0; i < LPC; ++i) load_one(q * LPC + i, wstep, base);            // tile s+1, in the MFMA shadow
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i][e], bv[cur][TN * e + j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (KCH > 0) {
            if ((s + 1) % KCH == 0 || s + 1 == nsteps) acc_close_chunk(tot, acc);      // wave-uniform
        }
        __syncthreads();
        store_lds();
        __syncthreads();
    }
    size_t pix_off[TN];
    bool pix_ok[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int oh = oh0 + (wn * TN + j) * RH + lcol / PT_C, ow = ow0 + lcol % PT_C;
        pix_ok[j] = oh < Ho && ow < Wo;
        pix_off[j] = pix_ok[j] ? (size_t)n * a.Cout * HWo + (size_t)oh * Wo + ow : 0;
    }
    if constexpr (KCH > 0)
        conv_epilogue<TM, TN, (TM > 1)>(tot, s_scale, s_shift, a.res, a.out, a.act, a.Cout, HWo, m0, wm, lrow, pix_off, pix_ok, m0 + BM <= a.Cout);
    else
        conv_epilogue<TM, TN, (TM > 1)>(acc, s_scale, s_shift, a.res, a.out, a.act, a.Cout, HWo, m0, wm, lrow, pix_off, pix_ok, m0 + BM <= a.Cout);
}

// (grouped, group.h; round 5: the single-pair trunk pass keeps ONE launch per layer, and a strided layer runs the same kernel --
// hence the same chunked sums -- whatever the batch it rides in)
template <int TM, int KCH = 0> using Direct3S2 = RfxFamily<C3Args, conv3x3_s2_body<TM, KCH>, 256, 2>;

template <int TM, int KCH = 0>
__global__ __launch_bounds__((Direct3S2<TM, KCH>::BLOCK), (Direct3S2<TM, KCH>::min_waves())) void conv3x3_s2_kernel(C3Args a) {
    conv3x3_s2_body<TM, KCH>(a, blockIdx.x, gridDim.x);
}

template <int TM, int PTC, bool FUSE, int TN, bool RAG, int KCH>
int launch_direct(C3Args& a, hipStream_t st) {
    using G = Patch<PTC, TN>;
    using F = Direct3<TM, PTC, FUSE, TN, RAG, KCH>;
    const long long rows = (long long)a.N * (a.H + 1);
    a.tilesM = (a.Cout + 64 * TM - 1) / (64 * TM);
    a.tilesH = (int)((rows + G::PT_R - 1) / G::PT_R);
    a.tilesW = (a.W + G::PT_C - 1) / G::PT_C;
    const long long nwg = (long long)a.tilesM * a.tilesH * a.tilesW;
    if (nwg > 0x7fffffffLL || rows > 0x7fffffffLL) return RFX_E_LIMIT;
    // 32-bit byte offsets inside the images one input patch can touch
    const long long span = (G::PR + a.H) / (a.H + 1) + 1;
    if (span * a.Cin * a.H * a.W * 4 > 0xffffffffLL) return RFX_E_LIMIT;
    if constexpr (TN == 2 && !RAG) return F::launch(conv3x3_direct_kernel<TM, PTC, FUSE, TN, RAG, KCH>, a, (unsigned)nwg, st);
    // the other instances have no grouped form: launched at once
    hipLaunchKernelGGL((conv3x3_direct_kernel<TM, PTC, FUSE, TN, RAG, KCH>), dim3((unsigned)nwg), dim3(F::BLOCK), 0, st, a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

template <int TM, int KCH>
int launch_s2(C3Args& a, hipStream_t st) {
    const int Ho = (a.H - 1) / 2 + 1, Wo = (a.W - 1) / 2 + 1;
    a.tilesM = (a.Cout + 64 * TM - 1) / (64 * TM);
    a.tilesH = (Ho + s2::PT_R - 1) / s2::PT_R;
    a.tilesW = (Wo + s2::PT_C - 1) / s2::PT_C;
    const long long nwg = (long long)a.tilesM * a.tilesH * a.tilesW * a.N;
    if (nwg > 0x7fffffffLL) return RFX_E_LIMIT;
    if ((long long)a.Cin * a.H * a.W * 4 > 0xffffffffLL) return RFX_E_LIMIT;                    // 32-bit byte offsets inside one image
    return Direct3S2<TM, KCH>::launch(conv3x3_s2_kernel<TM, KCH>, a, (unsigned)nwg, st);
}

// Every instance the library builds (conv_dispatch.h decides which one a launch takes), template arguments as the kernels take them
struct C3Entry {
    int key;
    int (*launch)(C3Args&, hipStream_t);
};
template <int TM, int PTC, bool FUSE, int TN, bool RAG, int KCH> constexpr ConvInstance direct_instance() {
    return FUSE ? ConvInstance::fused_tail(TM, PTC, KCH) : ConvInstance::direct3x3(TM, PTC, TN, RAG, KCH);
}
#define D(...) {direct_instance<__VA_ARGS__>().id(), &launch_direct<__VA_ARGS__>}
const C3Entry kDirect[] = {
    // <TM, PT_C, FUSE, TN, RAG, KCH>: plain, and in chunks of 4 K steps (288 k)
    D(2, 16, false, 2, false, 0), D(2, 8, false, 2, false, 0), D(2, 4, false, 2, false, 0),
    D(1, 16, false, 2, false, 0), D(1, 8, false, 2, false, 0), D(1, 4, false, 2, false, 0),
    D(2, 16, false, 2, false, 4), D(2, 8, false, 2, false, 4), D(2, 4, false, 2, false, 4),
    D(1, 16, false, 2, false, 4), D(1, 8, false, 2, false, 4), D(1, 4, false, 2, false, 4),
    // 256-pixel patches (64-channel tiles only)
    D(1, 16, false, 4, false, 0), D(1, 16, false, 4, false, 4),
    // ragged last K step (Cin % 8 != 0)
    D(2, 16, false, 2, true, 0), D(2, 8, false, 2, true, 0), D(2, 4, false, 2, true, 0),
    D(1, 16, false, 2, true, 0), D(1, 8, false, 2, true, 0), D(1, 4, false, 2, true, 0),
    // the fused Bottleneck tail
    D(2, 16, true, 2, false, 0), D(2, 8, true, 2, false, 0), D(2, 4, true, 2, false, 0),
    D(1, 16, true, 2, false, 0), D(1, 8, true, 2, false, 0), D(1, 4, true, 2, false, 0),
    D(2, 16, true, 2, false, 4), D(2, 8, true, 2, false, 4), D(2, 4, true, 2, false, 4),
    D(1, 16, true, 2, false, 4), D(1, 8, true, 2, false, 4), D(1, 4, true, 2, false, 4),
};
#undef D
#define S2(TM, KCH) {ConvInstance::direct3x3_s2(TM, KCH).id(), &launch_s2<TM, KCH>}
const C3Entry kStride2[] = {S2(2, 0), S2(1, 0), S2(2, 4), S2(1, 4)};
#undef S2

int launch_from(const C3Entry* e, C3Args& a, hipStream_t st) { return e ? e->launch(a, st) : RFX_E_ARG; }

}  // namespace

// Internal entry used by rfx_conv3x3_f32 (conv.hip); preconditions: conv_dispatch.h
int rfx_conv3x3_direct_launch(const ConvInstance& ci, const float* in, const float* wP, const float* scale, const float* shift,
                              const float* residual, float* out, int N, int Cin, int H, int W, int Cout, int Mpad, int act,
                              hipStream_t st) {
    C3Args a;
    a.in = in; a.wT = wP; a.scale = scale; a.shift = shift; a.res = residual; a.out = out;
    a.N = N; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.act = act; a.Mpad = Mpad;
    a.wT3 = a.scale3 = a.shift3 = nullptr; a.Cexp = a.Mpad3 = a.act3 = 0;
#ifdef RFX_TRACE
    a.trace = rfx_debug_trace_ptr();
#endif
    return launch_from(ci.family == CONV_DIRECT3 ? conv_find(kDirect, ci) : nullptr, a, st);
}

// Internal entry used by rfx_conv3x3_s2_f32 (conv.hip): the direct stride-2 kernel above
int rfx_conv3x3_s2_launch(const ConvInstance& ci, const float* in, const float* wP, const float* scale, const float* shift,
                          const float* residual, float* out, int N, int Cin, int H, int W, int Cout, int act, hipStream_t st) {
    C3Args a;
    a.in = in; a.wT = wP; a.scale = scale; a.shift = shift; a.res = residual; a.out = out;
    a.N = N; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.act = act; a.Mpad = (Cout + 127) / 128 * 128;
    a.wT3 = a.scale3 = a.shift3 = nullptr; a.Cexp = a.Mpad3 = a.act3 = 0;
#ifdef RFX_TRACE
    a.trace = nullptr;
#endif
    return launch_from(conv_find(kStride2, ci), a, st);
}

// Bottleneck tail in one kernel: out = act3(bn3(conv1x1(act2(bn2(conv3x3(in))))) + residual)  (model/resnet50.py:71-79,93-103).
// The 3x3 convolution must be direct-eligible (stride 1, pad 1, Cin % 8 == 0) with Cmid in {64, 128} so that one workgroup
// tile holds all of its channels; Cexp % 128 == 0.
// Kernel instance rfx_conv3x3_conv1x1_f32 launches (for a profiler-side caller; bits as rfx_conv2d_kernel_id).
extern "C" int rfx_conv3x3_conv1x1_kernel_id(int N, int H, int W, int Cmid) {
    return conv_decide_tail(conv_knobs(), N, H, W, Cmid, rfx_group_recording()).id();
}

extern "C" int rfx_conv3x3_conv1x1_f32(const float* in, const float* wP2, const float* scale2, const float* shift2, int act2,
                                       const float* wQ3, const float* scale3, const float* shift3, const float* residual,
                                       int act3, float* out, int N, int Cin, int H, int W, int Cmid, int Cexp, void* stream) {
    if (!in || !wP2 || !wQ3 || !scale3 || !shift3 || !out || N <= 0 || H <= 0 || W <= 0) return RFX_E_ARG;
    if (Cin <= 0 || Cin % 8 != 0 || (Cmid != 64 && Cmid != 128) || Cexp <= 0 || Cexp % 128 != 0) return RFX_E_ARG;
    if (reinterpret_cast<uintptr_t>(wQ3) & 15) return RFX_E_ARG;
    if (act2 == RFX_ACT_SIGMOID || act3 == RFX_ACT_SIGMOID) return RFX_E_ARG;
    C3Args a;
    a.in = in; a.wT = wP2; a.scale = scale2; a.shift = shift2; a.res = residual; a.out = out;
    a.N = N; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cmid; a.act = act2; a.Mpad = 128;
    a.wT3 = wQ3; a.scale3 = scale3; a.shift3 = shift3; a.Cexp = Cexp; a.Mpad3 = Cexp; a.act3 = act3;
#ifdef RFX_TRACE
    a.trace = rfx_debug_trace_ptr();
#endif
    // round 5: chunks of 4 K steps (288 k) in the 3x3 phase, like rfx_conv3x3_f32(k_chunk = 4)
    return launch_from(conv_find(kDirect, conv_decide_tail(conv_knobs(), N, H, W, Cmid, rfx_group_recording())), a, rfx_stream(stream));
}
