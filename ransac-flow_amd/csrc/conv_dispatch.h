// conv_dispatch.h -- which kernel instance an fp32 convolution runs as: one decision, on the host, as a pure function.
//
// The extern "C" entry points gather the geometry, the environment (conv_knobs()) and whether a grouped launch is recording
// (group.h), ask ONCE, and hand the ConvInstance to the family's launcher, which looks it up in that family's instance table:
// rfx_conv2d_f32 and every *_kernel_id ask conv_decide(), the fused tail conv_decide_tail(); rfx_conv3x3_f32 / rfx_conv3x3_s2_f32,
// whose caller has chosen the family, ask conv_direct3x3() / conv_direct3x3_s2(), the functions conv_decide() answers with for
// their geometries.  Host only and free of HIP headers: tests/host/conv_dispatch_walk.cpp builds it with a plain C++17 compiler.
#pragma once
#include <stddef.h>
#include <stdlib.h>

// ---------------------------------------------------------------------------------------------------------------- environment
// Every switch of the fp32 convolution dispatch, read once per process.  All of them are A/B switches for experiments.
struct ConvKnobs {
    int force_variant;   // RFX_CONV_FORCE_VARIANT=0/1/2: the implicit-GEMM tile whatever the launch size (unset: the rule)
    int ws;              // RFX_CONV_WS=1: the wave-specialised implicit-GEMM form on the 128- and 64x128 tiles (default: off)
    int direct;          // RFX_CONV_DIRECT=0: the host's choice never names the direct 3x3 kernels
    int s2;              // RFX_CONV_S2=0: ... never the direct stride-2 kernel
    int kmajor;          // RFX_CONV_1X1=0: 1x1 / stride 1 on the generic implicit-GEMM kernel
    int c1_chunk;        // RFX_C1_CHUNK=<min K> for the k-major kernel's chunked sums (0: never; 1: the default 512)
    int vecb;            // RFX_CONV_VECB=0: no 16-byte pixel-side loads
    int c3_chunk;        // RFX_C3_CHUNK=0: the direct 3x3 kernel's long-K layers as one chain
    int c3_s2_chunk;     // RFX_C3_S2_CHUNK=0: the same for the stride-2 kernel
    int c3_tail_chunk;   // RFX_C3_TAIL_CHUNK=0: the Bottleneck tails as round 4's chains
    int c3_wide;         // RFX_C3_WIDE=0: never the 256-pixel patch
    int group_uniform;   // RFX_GROUP_UNIFORM=0: a recording group keeps each problem's own patch shape
};

inline const ConvKnobs& conv_knobs() {
    static const ConvKnobs k = [] {
        auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        return ConvKnobs{env("RFX_CONV_FORCE_VARIANT", -1), env("RFX_CONV_WS", -1), env("RFX_CONV_DIRECT", 1), env("RFX_CONV_S2", 1),
                         env("RFX_CONV_1X1", 1), env("RFX_C1_CHUNK", 1), env("RFX_CONV_VECB", 1), env("RFX_C3_CHUNK", 1),
                         env("RFX_C3_S2_CHUNK", 1), env("RFX_C3_TAIL_CHUNK", 1), env("RFX_C3_WIDE", 1), env("RFX_GROUP_UNIFORM", 1)};
    }();
    return k;
}

// ------------------------------------------------------------------------------------------------------------------- instance
enum ConvFamily {
    CONV_GEMM,          // conv.hip:    conv2d_mfma_kernel<TM, TN, ONE, WS, VECB>
    CONV_KMAJOR,        // conv1x1.hip: conv1x1_kmajor_kernel<TM, VEC, KCH>
    CONV_DIRECT3,       // conv3x3.hip: conv3x3_direct_kernel<TM, PT_C, false, TN, RAG, KCH>
    CONV_DIRECT3_S2,    // conv3x3.hip: conv3x3_s2_kernel<TM, KCH>
    CONV_FUSED_TAIL,    // conv3x3.hip: conv3x3_direct_kernel<TM, PT_C, true, 2, false, KCH>
};

// A family and that family's template arguments (the members a family has no use for hold the values its maker below gives them).
struct ConvInstance {
    ConvFamily family;
    int tm, tn;          // 64-channel / 32-pixel MFMA sub-tiles per wavefront
    int patch_cols;      // PT_C of the direct 3x3 kernels: 16 / 8 / 4
    bool one, ws, vecb;  // implicit GEMM: 1x1 specialisation, wave-specialised form; + k-major: 16-byte pixel-side loads
    bool rag;            // direct 3x3: ragged last K step (Cin % 8 != 0)
    int kch;             // K steps per chunk of the chunked accumulation, 0: one chain

    static constexpr ConvInstance gemm(int tm, int tn, bool one, bool ws, bool vecb) { return {CONV_GEMM, tm, tn, 0, one, ws, vecb, false, 0}; }
    static constexpr ConvInstance kmajor(int tm, bool vec, int kch) { return {CONV_KMAJOR, tm, 2, 0, true, false, vec, false, kch}; }
    static constexpr ConvInstance direct3x3(int tm, int pc, int tn, bool rag, int kch) { return {CONV_DIRECT3, tm, tn, pc, false, false, false, rag, kch}; }
    static constexpr ConvInstance direct3x3_s2(int tm, int kch) { return {CONV_DIRECT3_S2, tm, 2, 16, false, false, false, false, kch}; }
    static constexpr ConvInstance fused_tail(int tm, int pc, int kch) { return {CONV_FUSED_TAIL, tm, 2, pc, false, false, false, false, kch}; }

    // The id of include/rfx_api.h (rfx_conv2d_kernel_id states the layout): the one place the library writes these bits.
    constexpr int id() const {
        const int small = tm == 2 ? 0 : 1;                                      // bit 0 of every family but the implicit GEMM
        const int patch = patch_cols == 16 ? 0 : (patch_cols == 8 ? 64 : 128);  // bits 6-7
        const int chunked = kch ? 16384 : 0;                                    // bit 14
        switch (family) {
            case CONV_GEMM: return (tm == 2 ? 0 : (tn == 2 ? 1 : 2)) | (one ? 4 : 0) | (ws ? 8 : 0) | (vecb ? 16 : 0);
            case CONV_KMAJOR: return 1024 | 4 | small | (vecb ? 16 : 0) | chunked;
            case CONV_DIRECT3: return 32 | small | patch | (tn == 4 ? 2048 : 0) | (rag ? 4096 : 0) | chunked;
            case CONV_DIRECT3_S2: return 8192 | small | chunked;
            default: return 512 | small | patch | chunked;
        }
    }
};

// One table per family: {id of the instance, its launcher} (within a family the id names the instance); the lookup is a scan of
// at most 32 integers, on the launch path of every convolution.
template <class E, size_t n> inline const E* conv_find(const E (&table)[n], const ConvInstance& ci) {
    const int key = ci.id();
    for (const E& e : table)
        if (e.key == key) return &e;
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------- rules
// Implicit-GEMM tile: the largest tile that still gives >= ~2 workgroups per CU (256 CUs).
// 0: 128x128 (conv2d_mfma_kernel<2,2>), 1: 64x128 (<1,2>), 2: 64x64 (<1,1>)
inline int conv_tile_variant(const ConvKnobs& k, int N, int Cout, int Hout, int Wout) {
    if (k.force_variant >= 0) return k.force_variant;
    const long long P = (long long)N * Hout * Wout;
    const long long b22 = (long long)((Cout + 127) / 128) * ((P + 127) / 128);
    const long long b12 = (long long)((Cout + 63) / 64) * ((P + 127) / 128);
    if (Cout > 64 && b22 >= 512) return 0;
    if (b12 >= 512 || P >= 8192) return 1;
    return 2;
}

// Patch shape of the direct 3x3 kernels for a batch of N H x W maps stacked as one tall map (conv3x3.hip): the fewest padded
// pixels (ties: the widest, whose row segments coalesce best).  The fused Bottleneck tail writes Cexp channels per pixel from a
// narrow patch in short row segments: measured on equal work its 16x8 patch is ~9 % and its 32x4 patch ~40 % slower than 8x16,
// while the plain 3x3 kernel is indifferent (scripts/ubench/conv_bench.py on the 25x33 ... 112x148 maps of the pyramid) -- hence
// the weights.
inline int conv3x3_patch_cols(const ConvKnobs& k, int N, int H, int W, bool fused, bool recording) {
    // grouped launches (group.h): ONE patch shape for every problem of the group, so that a layer is one launch and not
    // one per shape -- the group is latency-bound, a few padded pixels on the small maps cost less than a serial launch
    if (k.group_uniform && recording) return 16;
    int best = 16;
    long long best_cost = -1;
    for (int pc = 16; pc >= 4; pc >>= 1) {
        const int pr = 128 / pc;
        const long long area = (((long long)N * (H + 1) + pr - 1) / pr) * ((W + pc - 1) / pc);
        const long long cost = area * (!fused || pc == 16 ? 100 : (pc == 8 ? 109 : 140));
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = pc; }
    }
    return best;
}

// 256-pixel (16 x 16) patches for a layer whose output channels fit ONE 64-channel tile: only for launches that still fill the
// chip two generations deep with the larger patch, never inside a grouped launch (latency-bound: more, smaller workgroups win).
inline bool conv3x3_wide_patch(const ConvKnobs& k, int N, int H, int W, int Cout, int patch_cols, bool recording) {
    if (!k.c3_wide || recording || patch_cols != 16 || Cout > 64) return false;
    const long long tiles = (((long long)N * (H + 1) + 15) / 16) * ((W + 15) / 16);
    return tiles >= 1024;
}

// The instance rfx_conv3x3_f32 launches: 3x3 / stride 1 / pad 1, Cin >= 8, weights in the kernel's own packed order.
inline ConvInstance conv_direct3x3(const ConvKnobs& k, int N, int Cin, int Cout, int H, int W, int k_chunk, bool recording) {
    const int pc = conv3x3_patch_cols(k, N, H, W, false, recording), pr = 128 / pc;
    const long long tiles = (((long long)N * (H + 1) + pr - 1) / pr) * ((W + pc - 1) / pc);
    // RFX_CONV_DIRECT=0 only changes the host's choice: a caller that still comes here gets the plain kernel, tiled by Cout alone
    const bool big = Cout > 64 && (!k.direct || tiles * ((Cout + 127) / 128) >= 512);
    const bool rag = Cin % 8 != 0;   // ragged last K step: separate instances (never recorded into a grouped launch: launched at once)
    // Chunked accumulation (KCH in conv3x3.hip) for the layers whose single fma chain is longest: K = 9 Cin >= 2048 (RFX_C3_CHUNK=0
    // turns it off for A/B runs: the chain form is what rfx_conv2d_f32's implicit-GEMM kernel computes) -- or asked for by the
    // caller (k_chunk > 0: the 3x3 convolution of a Bottleneck tail, K = 576 / 1152, run on its own; RFX_C3_TAIL_CHUNK=0: the
    // round-4 chains).  A single image / tiny batch runs the long-K layers on 64-channel tiles: same chunks.
    const bool chk = k.direct && !rag && ((k.c3_chunk && Cin * 9 >= 2048) || (k_chunk > 0 && k.c3_tail_chunk));
    const bool wide = !rag && conv3x3_wide_patch(k, N, H, W, Cout, pc, recording);
    return ConvInstance::direct3x3(big ? 2 : 1, pc, wide ? 4 : 2, rag, chk ? 4 : 0);
}

// Whether the library's own rule takes the direct 3x3 / stride 2 / pad 1 kernel (Cin % 8 == 0).
// Its 8 x 16 output patches tile every image on their own (no stacked-batch trick at stride 2): on maps that pad badly
// the implicit-GEMM kernel, which tiles the flattened pixel axis, wins.  Measured break-even (scripts/ubench/
// conv_s2_bench.py, profiles/r04_conv_s2_ab.json): +8..16 % at 100 % / 94 % useful pixels, +-0 at 88 %, -12 % at 74 %.
// Round 5: the layers with K = 9 Cin >= 1152 sum in chunks of 4 K steps (288 products) in this kernel, like the stride-1
// kernel (RFX_C3_S2_CHUNK=0: chains) -- they take it on EVERY map and inside grouped launches too, so that a layer's sums
// never depend on the map size or the batch; the shorter-K layers keep the rule above and, while a group records, the
// implicit-GEMM kernel (either kernel: the same chain, bit-identical).
inline bool conv_s2_chunked(const ConvKnobs& k, int Cin) { return k.c3_s2_chunk && Cin * 9 >= 1152; }
inline bool conv_s2_preferred(const ConvKnobs& k, int Cin, int Hout, int Wout, bool recording) {
    const long long th = (Hout + 7) / 8, tw = (Wout + 15) / 16;
    return k.direct && k.s2 && (conv_s2_chunked(k, Cin) || ((long long)Hout * Wout * 100 >= 90 * th * 8 * tw * 16 && !recording));
}
// The instance rfx_conv3x3_s2_f32 launches; a caller that comes here against the rule gets its tile by Cout alone.
inline ConvInstance conv_direct3x3_s2(const ConvKnobs& k, int N, int Cin, int Cout, int Hout, int Wout, bool recording) {
    const long long tiles = (long long)N * ((Hout + 7) / 8) * ((Wout + 15) / 16);
    const bool big = Cout > 64 && (!conv_s2_preferred(k, Cin, Hout, Wout, recording) || tiles * ((Cout + 127) / 128) >= 512);
    return ConvInstance::direct3x3_s2(big ? 2 : 1, conv_s2_chunked(k, Cin) ? 4 : 0);
}

struct ConvGeom {
    int N, Cin, Cout, KH, KW, stride, pad, Hout, Wout;
};

// The instance a convolution of this geometry runs as.  allow_direct: the caller holds the packed weights of the direct 3x3
// kernels (rfx_conv2d_f32 itself does not: it always runs the implicit GEMM or the k-major 1x1 kernel); k_chunk: rfx_conv3x3_f32's
// argument; in_aligned: the input pointer is 16-byte aligned (an id query knows no pointer and says true); recording: a grouped
// launch is recording (group.h).
inline ConvInstance conv_decide(const ConvKnobs& k, const ConvGeom& g, bool allow_direct, int k_chunk, bool in_aligned, bool recording) {
    const bool k3 = allow_direct && k.direct && g.KH == 3 && g.KW == 3 && g.pad == 1 && g.Cin >= 8;
    if (k3 && g.stride == 1) return conv_direct3x3(k, g.N, g.Cin, g.Cout, g.Hout, g.Wout, k_chunk, recording);
    if (k3 && g.stride == 2 && g.Cin % 8 == 0 && conv_s2_preferred(k, g.Cin, g.Hout, g.Wout, recording))
        return conv_direct3x3_s2(k, g.N, g.Cin, g.Cout, g.Hout, g.Wout, recording);
    const int variant = conv_tile_variant(k, g.N, g.Cout, g.Hout, g.Wout);
    const bool one = g.KH == 1 && g.KW == 1 && g.pad == 0;
    const long long HW = (long long)g.Hout * g.Wout;
    // 16-byte pixel-side loads: 1x1, stride 1, whole planes of a multiple of 4 pixels that start 16-byte aligned
    const bool vec = one && g.stride == 1 && HW % 4 == 0 && in_aligned;
    // k-major 1x1 / stride 1 kernel (conv1x1.hip).  Chunked accumulation from K = 512 on (layer2 conv1, layer3.0 conv1: two chunks of
    // 256; conv1x1_kmajor_kernel<1, VEC, 8>, 64-channel tiles, at EVERY launch size -- a result must not depend on how many pairs
    // share the launch).
    const bool chk = k.c1_chunk && g.Cin >= (k.c1_chunk > 1 ? k.c1_chunk : 512);
    if (k.kmajor && one && g.stride == 1 && g.Cin % 32 == 0 && g.Cin >= 64 && (variant != 2 || chk) && g.N * HW >= 4)
        return ConvInstance::kmajor(chk || variant ? 1 : 2, vec, chk ? 8 : 0);
    // The wave-specialised form pays off where the gather is the heavy part and the K loop is long: KxK (K > 1) convolutions on the
    // 128x128 tile (measured +5 % there, -5...-15 % on 1x1 and 64-wide tiles, which keep the single-role kernel with two
    // independent workgroups per CU).  Off by default: since the branch-free epilogue the single-role kernel is as fast.
    const bool ws = variant < 2 && k.ws > 0;
    return ConvInstance::gemm(variant == 0 ? 2 : 1, variant < 2 ? 2 : 1, one, ws, k.vecb && vec && !ws);
}

// The instance of the fused Bottleneck tail rfx_conv3x3_conv1x1_f32 (Cmid in {64, 128}: one workgroup tile holds all mid channels).
// The 256-pixel patch buys the fused tail nothing (100.9 vs 100.5 TFLOP/s): its loss is the expansion phase.
inline ConvInstance conv_decide_tail(const ConvKnobs& k, int N, int H, int W, int Cmid, bool recording) {
    return ConvInstance::fused_tail(Cmid == 64 ? 1 : 2, conv3x3_patch_cols(k, N, H, W, true, recording), k.c3_tail_chunk ? 4 : 0);
}

// ------------------------------------------------------------- launchers across the files (conv3x3.hip, conv1x1.hip)
typedef struct ihipStream_t* hipStream_t;   // as the HIP runtime declares it

// Preconditions, checked by the caller: ci is of the launcher's family and was decided for this geometry and this `in`.
int rfx_conv3x3_direct_launch(const ConvInstance& ci, const float* in, const float* wP, const float* scale, const float* shift,
                              const float* residual, float* out, int N, int Cin, int H, int W, int Cout, int Mpad, int act,
                              hipStream_t st);
int rfx_conv3x3_s2_launch(const ConvInstance& ci, const float* in, const float* wP, const float* scale, const float* shift,
                          const float* residual, float* out, int N, int Cin, int H, int W, int Cout, int act, hipStream_t st);
int rfx_conv1x1_kmajor_launch(const ConvInstance& ci, const float* in, const float* wT, const float* scale, const float* shift,
                              const float* residual, float* out, int N, int Cin, int HW, int Cout, int Mpad, int act,
                              hipStream_t st);
