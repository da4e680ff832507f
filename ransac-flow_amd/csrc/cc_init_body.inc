// Body of the run-link kernels (cc.hip).  The including kernel has set in, parent, area (at the first pixel it owns), total = the
// number of pixels it owns, W = their row width and th.
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < total; base += stride) {
        const long long i = base + lane;
        const bool ok = i < total;
        const bool fg = ok && in[i] > th;
        const int x = ok ? (int)(i % W) : 0;
        const unsigned long long m = __ballot(fg);
        // left neighbour foreground and in the same row?  (lane 0 looks into the previous segment)
        const bool left = fg && x > 0 && (lane > 0 ? ((m >> (lane - 1)) & 1ull) != 0 : in[i - 1] > th);
        const unsigned long long starts = __ballot(fg && !left) | (m & 1ull);   // run starts inside the segment (+ lane 0)
        if (ok) {
            int par = -1;
            if (fg) {
                const unsigned long long below = starts & (~0ull >> (63 - lane));    // start bits at or below this lane
                const int s = 63 - __clzll((long long)below);                          // below != 0: lane 0 is always a start bit
                par = (lane == 0 && left) ? (int)(i - 1) : (int)(base + s);
            }
            parent[i] = par;
            area[i] = 0;
        }
    }
