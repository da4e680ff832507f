// conv_split.h -- what the split-arithmetic convolution kernels share (conv1x1s.hip, conv3x3s.hip): float32 results on the bf16 matrix
// pipe by EXACT operand splitting (round 6; the Bottleneck conv1 / conv3 layers of the ResNet-50 trunk, model/resnet50.py:71-79,93-103,
// and the 3x3 layers of conv3x3s.hip).
//
// A float32 x has a 24-bit significand = three bf16 pieces of 8 bits:  x = hi + mid + lo  EXACTLY, with hi = bf16(x) (round to
// nearest even), mid = bf16(x - hi), lo = bf16(x - hi - mid) (both differences are exact in float32).  A product of two pieces
// (8 x 8 bits) is exact in float32, so
//     w * x = (wh + wm + wl)(xh + xm + xl) = wh xh + [wh xm + wm xh] + [wm xm + wh xl + wl xh] + (three terms below 2^-24 (1 + 2^-10) |w x|)
// and six v_mfma_f32_32x32x16_bf16 per 16 k give the float32 sum with EVERY product exact -- what differs from an fp32 fma chain is
// only where the float32 accumulator rounds: the matrix core adds the 16 products of an instruction before it rounds, and the hi*hi
// products run in their own accumulator (the five small terms in a second one, added once at the end).  Measured on convolution-
// shaped data (scripts/ubench/bf16x_emul.hip, profiles/r06_bf16_split_study.json): rms error against the float64 sum 2.3e-7 of the
// output rms at K = 2304, against 6.1e-7 for the fp32 MFMA's single fma chain and 3.0e-7 for the chunked chain the fp32 kernels use
// -- CLOSER to the exact sum IN RMS than the float32 kernels it replaces, at 2.1x their matrix-pipe rate (6 x 32 cycles against 8 x 64
// per 16 k).  Not in the max error at long K: against the chunked fp32 kernels the worst element is 1.2x - 2.9x further off at
// K = 2304 / 4608 (the hi*hi accumulator is one chain of K / 16 roundings; profiles/split_max_error_ratio.json; the tests bound the
// ratio and hold every element to a rigorous bound).  The dropped terms: at most 2^-24 (1 + 2^-10) |w x|, nearly attained (tests/test_split_numerics_cpu.py).
// Not bit-identical to the fp32 kernels (conv1x1.hip stays: rfx_conv2d_f32 never routes here; the caller asks for a split entry point).
// Infinities: x = +-inf gives hi = inf, x - hi = NaN -> NaN where the fp32 kernel returns +-inf (NaN inputs give NaN in both).
//
// Weights are split ONCE on the host into the three pieces and packed in fragment order (rfx_api.h: "wS" / "wS3"): per stage q (a
// 16-k block; conv3x3s.hip: a (block, tap) pair)
//     wS[q][piece][h = (k % 16) / 8][m (Mpad)][8 bf16]      -- a lane's A fragment (row m, k = 16 kb + 8 h .. + 7) = one 16-byte word
// and a workgroup's stage image in LDS is As[piece][h][BM] (SplitWeights below).  Activations are float32 in HBM as everywhere: the
// staging threads split 8 (or 4) consecutive k of one pixel (split_word: v_cvt_pk_bf16_f32 + v_pk_add_f32, 4.5 vector-ALU
// instructions per element) into 16-byte words Bs[piece][h][pixel][8 bf16], so that both fragments of an MFMA are single conflict-free
// ds_read_b128.  The order of the six products of a stage, its sched_barriers and waits are each kernel's own.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

static __device__ __forceinline__ unsigned pack_bf16(float a, float b) {      // (bf16(a) | bf16(b) << 16), round to nearest even: v_cvt_pk_bf16_f32
    const f32x2 v = {a, b};
    const bf16x2 h = __builtin_convertvector(v, bf16x2);
    unsigned u;
    __builtin_memcpy(&u, &h, 4);
    return u;
}
// two float32 -> their three bf16 pieces, packed pairwise
static __device__ __forceinline__ void split_pair(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
    hi = pack_bf16(a, b);
    const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);            // exact
    mid = pack_bf16(ra, rb);
    lo = pack_bf16(ra - __uint_as_float(mid << 16), rb - __uint_as_float(mid & 0xffff0000u));
}
static __device__ __forceinline__ bf16x8 as_frag(const u32x4& w) {
    bf16x8 f;
    __builtin_memcpy(&f, &w, 16);
    return f;
}
// 2 N consecutive k of one pixel -> N packed pairs of each piece; V = u32x4 (8 floats -> one 16-byte word per piece) or u32x2
template <typename V>
static __device__ __forceinline__ void split_word(const float* v, V& hi, V& mid, V& lo) {
#pragma unroll
    for (int i = 0; i < (int)(sizeof(V) / 4); ++i) {
        unsigned h_, m_, l_;
        split_pair(v[2 * i], v[2 * i + 1], h_, m_, l_);
        hi[i] = h_; mid[i] = m_; lo[i] = l_;
    }
}

// Staging roles of a stage's weight image through registers (conv1x1s.hip; conv3x3s.hip's stride-1 body with ADMA off), NT threads:
// words t + NT j (j < NA) of As[piece][h][BM] <- wS[q][piece][h][m0 + m].  NT words = ROWS [piece][h] rows: word t + NT j sits
// ROWS * j rows below word t.
template <int BM, int NT>
struct SplitWeights {
    static constexpr int WORDS = 3 * 2 * BM;            // 16-byte words of a stage image
    static constexpr int NA = (WORDS + NT - 1) / NT;    // per thread
    static constexpr int ROWS = NT / BM;
    const u32x4* src;                                   // + (q * 6 + ROWS * j) * Mpad (an argument, not a member: a copy costs registers)
    u32x4 ra[NA];

    // clamp_rows: the tile may end past Mpad (conv1x1s.hip's 256-channel tile: Mpad is a multiple of 128) -- those lanes read the last
    // row instead (any valid word: their outputs are channels >= Cout, which the epilogue does not store)
    __device__ __forceinline__ void init(const u32x4* wS, int Mpad, int m0, bool clamp_rows = false) {
        const int t = threadIdx.x;
        src = wS + (size_t)(t / BM) * Mpad + m0 + t % BM;
        if (clamp_rows && m0 + t % BM >= Mpad) src = wS + (size_t)(t / BM) * Mpad + Mpad - 1;
    }
    // word j exists for every thread (compile time) or for the first wavefronts only (64-channel tiles: 384 words): no per-lane branches
    // around the loads -- a divergent region makes the compiler drain the vector-memory counter between two loads
    __device__ __forceinline__ bool on(int j) const { return (j + 1) * NT <= WORDS || (int)threadIdx.x + NT * j < WORDS; }
    __device__ __forceinline__ void load(int q, int Mpad) {       // stage q -> registers
#pragma unroll
        for (int j = 0; j < NA; ++j) ra[j] = src[((size_t)q * 6 + (on(j) ? ROWS * j : 0)) * Mpad];       // off lanes: any valid word
    }
    __device__ __forceinline__ void store(u32x4* img) const {      // registers -> the stage image
        const int t = threadIdx.x;
#pragma unroll
        for (int j = 0; j < NA; ++j)
            if (on(j)) img[t + NT * j] = ra[j];
    }
};

// argument checks the split entry points share
static inline int conv_check_common(const void* in, const void* w, const void* out, int N, int Cin, int H, int W, int Cout, int act) {
    if (!in || !w || !out || N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return RFX_E_ARG;
    if (Cin % 16 != 0) return RFX_E_ARG;
    if (act != RFX_ACT_NONE && act != RFX_ACT_RELU && act != RFX_ACT_SIGMOID) return RFX_E_ARG;
    return RFX_OK;
}
