// Per-workgroup set-up shared by the MFMA convolution kernels (conv.hip, conv1x1.hip, conv1x1s.hip, conv3x3.hip, conv3x3s.hip):
// what stands in front of conv_epilogue.h and does not depend on the kernel family.  The __shared__ arrays are declared in the
// kernel bodies; the helpers take pointers.
#pragma once
#include "common.h"

// folded BatchNorm of the tile's BM output channels m0 .. m0 + BM - 1 -> LDS (visible after the next barrier); channels past Cout
// and absent vectors read as the identity
template <int BM>
static __device__ __forceinline__ void stage_bn(float* s_scale, float* s_shift, const float* scale, const float* shift, int m0, int Cout) {
    const int t = threadIdx.x;
    if (t < BM) {
        const int m = m0 + t;
        s_scale[t] = (scale && m < Cout) ? scale[m] : 1.0f;
        s_shift[t] = (shift && m < Cout) ? shift[m] : 0.0f;
    }
}

// the accumulator tiles of a wavefront: TM x TN MFMA sub-tiles of 32 x 32
template <int TM, int TN>
static __device__ __forceinline__ void acc_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
}
template <int TM, int TN>
static __device__ __forceinline__ void acc_add(f32x16 (&acc)[TM][TN], const f32x16 (&low)[TM][TN]) {      // acc += low
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] += low[i][j][r];
}
// chunked accumulation (conv3x3.hip): the chunk's sum joins the total and the chain restarts from zero
template <int TM, int TN>
static __device__ __forceinline__ void acc_close_chunk(f32x16 (&tot)[TM][TN], f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { tot[i][j][r] += acc[i][j][r]; acc[i][j][r] = 0.0f; }
}

// Epilogue pixel offsets (conv_epilogue.h: pix_off / pix_ok) of this lane's pixel in each of its TN 32-pixel sub-tiles, for kernels
// that number the output pixels of the batch 0 .. P - 1, HW per image; p0 = this lane's pixel of sub-tile 0.  Columns past the end
// get a valid offset (the last pixel's) and pix_ok = false.  The 3x3 kernels' stacked-rows forms stay in their bodies.
template <int TN>
static __device__ __forceinline__ void pix_linear(size_t (&pix_off)[TN], bool (&pix_ok)[TN], long long p0, long long P, int HW, int Cout) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        long long pp = p0 + j * 32;
        pix_ok[j] = pp < P;
        if (!pix_ok[j]) pp = P - 1;
        const long long n = pp / HW;
        pix_off[j] = (size_t)n * Cout * (size_t)HW + (size_t)(pp - n * HW);
    }
}
