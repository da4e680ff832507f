// Body of the accept-statistic kernels (multih.hip): partial blockIdx.x of NPART over pair k's HW pixels.  The including kernel has
// set k, b, HW and defines MH_MATCH_OFF / MH_MASK_OFF (element offsets of the pair's matchability map and mask).
    match += MH_MATCH_OFF; mask += MH_MASK_OFF;
    if (bg) bg += MH_MASK_OFF;
    const long long per = (HW + NPART - 1) / NPART;
    const long long p0 = blockIdx.x * per, p1 = p0 + per < HW ? p0 + per : HW;
    double s = 0.0;
    for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
        const float nf = __fsub_rn(1.0f, fg_px(mask, bg, (size_t)p));
        const float m = match[p];
        s += (double)__fmul_rn(mode ? (m > 0.9999f ? 1.0f : 0.0f) : m, nf);
    }
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)k * NPART + blockIdx.x] = red[0];
