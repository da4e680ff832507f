// Body of the compaction kernels (mutual_nn.hip), included like mnn_tile_kmajor_body.inc.  Expects in scope: MnnArgs a.
    char* ws = a.ws + (size_t)blockIdx.x * a.wsStride;
    const float* rowVal = reinterpret_cast<const float*>(ws + a.oRowVal);
    const int* rowIdx = reinterpret_cast<const int*>(ws + a.oRowIdx);
    const int* colIdx = reinterpret_cast<const int*>(ws + a.oColIdx);
    const int nA = a.nA, nB = a.nB;
    int64_t* idx1 = a.idx1 + (size_t)blockIdx.x * a.idxStride;
    int64_t* idx2 = a.idx2 + (size_t)blockIdx.x * a.idxStride;
    int32_t* count = a.count + blockIdx.x;
    __shared__ int wsum[16];
    __shared__ int base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) base = 0;
    __syncthreads();
    for (int s = 0; s < nA; s += 1024) {
        const int i = s + t;
        bool keep = false;
        int j = 0;
        if (i < nA) {
            j = rowIdx[i];
            const float v = rowVal[i];
            keep = ((unsigned)j < (unsigned)nB) && (colIdx[j] == i) && (v * v > 0.0f);
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 16; ++w) {
            const int c = wsum[w];
            if (w < wave) woff += c;
            tot += c;
        }
        const int b = base;
        if (keep) {
            idx1[b + woff + before] = i;
            idx2[b + woff + before] = j;
        }
        __syncthreads();
        if (t == 0) base = b + tot;
        __syncthreads();
    }
    if (t == 0) count[0] = base;
