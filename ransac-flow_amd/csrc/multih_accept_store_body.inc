// Body of the record-store kernels (multih.hip).  The including kernel has set k, b, hw8, hwd2, the record offsets and defines
// MH_F8_OFF / MH_M8_OFF / MH_D2_OFF (element offsets of pair k's /8 flow, /8 matchability maps and half-resolution flow).
    if (!accept[k]) return;
    const int slot = nbH[b];
    const int t = threadIdx.x;
    if (rec && slot < max_h) {
        float* r = rec + (size_t)b * rec_stride;
        if (t < 9) r[off_H + slot * 9 + t] = bestH[k * 9 + t];
        if (flow8)
            for (int i = t; i < 2 * hw8; i += 1024) r[off_flow + (size_t)slot * 2 * hw8 + i] = flow8[MH_F8_OFF + i];
        if (m12 && m21)
            for (int i = t; i < hw8; i += 1024) {
                r[off_match + (size_t)slot * 2 * hw8 + i] = m12[MH_M8_OFF + i];
                r[off_match + (size_t)slot * 2 * hw8 + hw8 + i] = m21[MH_M8_OFF + i];
            }
        if (flowd2)
            for (int i = t; i < 2 * hwd2; i += 1024) r[off_d2 + (size_t)slot * 2 * hwd2 + i] = flowd2[MH_D2_OFF + i];
    }
    __syncthreads();
    if (t == 0) {
        nbH[b] = slot + 1;
        // the record's nbH field never exceeds the slots it holds; a pair that accepted more (only the unbounded KITTI loop
        // can) is flagged with status 3, and the device counter nbH[] keeps the true number
        if (rec) {
            rec[(size_t)b * rec_stride] = (float)(slot + 1 < max_h ? slot + 1 : max_h);
            rec[(size_t)b * rec_stride + 1] = slot + 1 > max_h ? 3.0f : 0.0f;
        }
    }
