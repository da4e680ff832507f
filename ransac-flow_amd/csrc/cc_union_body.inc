// Body of the union kernels (cc.hip).  The including kernel has set parent (at the first pixel it owns), total and H, W = the
// size of one image.
    const long long HW = (long long)H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        if (cc_ld(parent + i) < 0) continue;
        const long long p = i % HW;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        if (y == 0) continue;
        const bool w = x > 0 && cc_ld(parent + i - 1) >= 0;
        const bool e = x + 1 < W && cc_ld(parent + i + 1) >= 0;
        const bool n = cc_ld(parent + i - W) >= 0;
        const bool nw = x > 0 && cc_ld(parent + i - W - 1) >= 0;
        const bool ne = x + 1 < W && cc_ld(parent + i - W + 1) >= 0;
        if (n && !(w && nw)) cc_unite(parent, (int)i, (int)(i - W));
        if (nw && !w && !n) cc_unite(parent, (int)i, (int)(i - W - 1));
        if (ne && !n && !e) cc_unite(parent, (int)i, (int)(i - W + 1));
    }
