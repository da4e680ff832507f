// Body of the accept-rule / mask-update kernels (multih.hip).  The including kernel has set k, b, HW and defines MH_MATCH_OFF /
// MH_MASK_OFF.
    __shared__ int s_acc;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int q = 0; q < NPART; ++q) s += part[(size_t)k * NPART + q];     // fixed order: every block gets the same sum
        const float g = (float)(s / (double)HW);
        const bool ok = n_match[k] >= 4 && res[k * 4] == 0 && ((double)g > th || nbH[b] == 0);
        s_acc = ok ? 1 : 0;
        if (blockIdx.x == 0) { accept[k] = ok ? 1 : 0; gain[k] = g; }
    }
    __syncthreads();
    if (!s_acc) return;
    match += MH_MATCH_OFF; mask += MH_MASK_OFF;
    if (bg) bg += MH_MASK_OFF;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
        const float mk = mask[p];
        const float bgv = bg ? bg[p] : 1.0f;
        const float fg = __fadd_rn(mk, __fsub_rn(1.0f, bgv)) > 0.5f ? 1.0f : 0.0f;
        const float v = __fadd_rn(mk, __fmul_rn(match[p], __fsub_rn(1.0f, fg)));
        mask[p] = (mode ? v > 0.9999f : v >= 1.0f) ? 1.0f : 0.0f;
    }
