// Body of the match-filter kernels (multih.hip): ordered ballot compaction of one pair's cached matches.  The including kernel has set
// k, n, h, w, ct, sh, sw, cap and moved mask / bg / idx1 / idx2 / xa / ya / xb / yb / m1 / m2 / kept to the pair.
    __shared__ int wsum[16];
    __shared__ int base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) base = 0;
    __syncthreads();
    for (int s = 0; s < n; s += 1024) {
        const int i = s + t;
        bool keep = false;
        int64_t a = 0, cell = 0;
        if (i < n) {
            a = idx1[i]; cell = idx2[i];
            const int r = (int)(cell / ct), c = (int)(cell - (int64_t)r * ct);
            keep = keep_cell(mask, bg, h, w, sh, sw, r, c);
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) { const int cq = wsum[q]; if (q < wave) woff += cq; tot += cq; }
        const int b0 = base;
        if (keep) {
            const size_t o = (size_t)(b0 + woff + before) * 3;
            m1[o] = xa[a]; m1[o + 1] = ya[a]; m1[o + 2] = 1.0f;
            m2[o] = xb[cell]; m2[o + 1] = yb[cell]; m2[o + 2] = 1.0f;
            if (kept) kept[b0 + woff + before] = i;
        }
        __syncthreads();
        if (t == 0) base = b0 + tot;
        __syncthreads();
    }
    const int ntot = base;
    for (int i = ntot + t; i < cap; i += 1024) {
        const size_t o = (size_t)i * 3;
        m1[o] = m1[o + 1] = m1[o + 2] = 0.0f;
        m2[o] = m2[o + 1] = m2[o + 2] = 0.0f;
        if (kept) kept[i] = -1;
    }
    if (t == 0) n_out[k] = ntot;
