// Body of the reduce kernels (mutual_nn.hip), included like mnn_tile_kmajor_body.inc.  Expects in scope: MnnArgs a.
    char* ws = a.ws + (size_t)blockIdx.y * a.wsStride;
    const float* rowPartVal = reinterpret_cast<const float*>(ws + a.oRowPartVal);
    const int* rowPartIdx = reinterpret_cast<const int*>(ws + a.oRowPartIdx);
    const float* colPartVal = reinterpret_cast<const float*>(ws + a.oColPartVal);
    const int* colPartIdx = reinterpret_cast<const int*>(ws + a.oColPartIdx);
    float* rowVal = reinterpret_cast<float*>(ws + a.oRowVal);
    int* rowIdx = reinterpret_cast<int*>(ws + a.oRowIdx);
    int* colIdx = reinterpret_cast<int*>(ws + a.oColIdx);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < a.nA) {
        float bv = -INFINITY;
        int bj = 0x7fffffff;
        for (int tb = 0; tb < a.tilesB; ++tb)
            take_min_idx(bv, bj, rowPartVal[(size_t)tb * a.nA + g], rowPartIdx[(size_t)tb * a.nA + g]);
        rowVal[g] = bv;
        rowIdx[g] = bj;
    } else if (g - a.nA < a.nB) {
        const int j = g - a.nA;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int ta = 0; ta < a.tilesA; ++ta)
            take_min_idx(bv, bi, colPartVal[(size_t)ta * a.nB + j], colPartIdx[(size_t)ta * a.nB + j]);
        colIdx[j] = bi;
    }
