// Body of the label / area kernels (cc.hip).  The including kernel has set parent, label, area (at the first pixel it owns) and total.
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < total; base += stride) {
        const long long i = base + (threadIdx.x & 63);
        int r = -1;
        if (i < total) {
            if (cc_ld(parent + i) >= 0) r = cc_find(parent, (int)i);
            label[i] = r;
        }
        unsigned long long todo = __ballot(r >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lr = __shfl(r, leader);
            const unsigned long long same = __ballot(r == lr) & todo;
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(&area[lr], __popcll(same));
            todo &= ~same;
        }
    }
