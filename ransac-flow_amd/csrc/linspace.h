// torch.linspace(-1, 1, n)[i] as ATen's CPU kernel computes it, bit for bit: step = 2 / (n - 1) in float32, the lower half counted up
// from -1 and the upper half counted down from 1 (symmetric about the midpoint), each as ONE fused multiply-add.  The fmaf is spelled
// out so that a translation unit built with -ffp-contract=off (epe.hip) gets the value warp.hip gets: the identity grid every flow of
// the fine stage was added to.
#pragma once
#include <hip/hip_runtime.h>

static __device__ __forceinline__ float rfx_lin(int i, int n) {
    if (n <= 1) return -1.0f;
    const float step = 2.0f / (float)(n - 1);
    return i < n / 2 ? fmaf(step, (float)i, -1.0f) : fmaf(-step, (float)(n - 1 - i), 1.0f);
}
