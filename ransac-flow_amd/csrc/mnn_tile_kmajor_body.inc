// Body of the k-major tile kernels (mutual_nn.hip): included, not called, so that mnn_tile_kmajor_kernel compiles from exactly
// this text.  Expects in scope: MnnArgs a, template parameters VEC and WA.
    constexpr int BMA = BM * WA, NT = 256 * WA;
    constexpr int A_TPR = VEC ? BMA / 4 : BMA;     // threads per A row
    constexpr int A_RPR = NT / A_TPR;              // A rows per round of all threads: 8 (VEC) / 2 (scalar)
    constexpr int NLA = BK / A_RPR;                // A loads per thread and K step: 4 / 16
    constexpr int B_TPR = VEC ? BN / 4 : BN;
    constexpr int B_RPR = NT / B_TPR;              // 8 * WA / 2 * WA
    constexpr int NLB = BK / B_RPR;                // 4 / WA, 16 / WA
    __shared__ __attribute__((aligned(16))) float As[2][BK][BMA];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = lane >> 5, lcol = lane & 31;
    const int pair = blockIdx.y;
    const float* Ab = a.A + (size_t)pair * a.strideA;
    const float* Bb = a.B + (size_t)pair * a.strideB;
    char* ws = a.ws + (size_t)pair * a.wsStride;
    float* rowPartVal = reinterpret_cast<float*>(ws + a.oRowPartVal);
    int* rowPartIdx = reinterpret_cast<int*>(ws + a.oRowPartIdx);
    float* colPartVal = reinterpret_cast<float*>(ws + a.oColPartVal);
    int* colPartIdx = reinterpret_cast<int*>(ws + a.oColPartIdx);
    const int nwg = a.tilesA * a.tilesB;
    int bid = blockIdx.x;
    {   // XCD-aware bijective remap; column tile fastest so an XCD's L2 keeps one A panel hot
        const int q = nwg / 8, r = nwg % 8, xcd = bid % 8, j = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    }
    const int tb = bid % a.tilesB, ta = bid / a.tilesB;
    const int i0 = ta * BMA, j0 = tb * BN;
    // staging roles: row t / TPR (+ RPR per round), cells (t % TPR) * (VEC ? 4 : 1) ..
    const int arow_s = t / A_TPR, acol_s = (t % A_TPR) * (VEC ? 4 : 1);
    const int brow_s = t / B_TPR, bcol_s = (t % B_TPR) * (VEC ? 4 : 1);
    int ca = i0 + acol_s, cb = j0 + bcol_s;
    if (VEC) { if (ca + 4 > a.ldA) ca = a.ldA - 4; if (cb + 4 > a.ldB) cb = a.ldB - 4; }
    else     { if (ca >= a.nA) ca = a.nA - 1;     if (cb >= a.nB) cb = a.nB - 1; }
    const float* asrc = Ab + (size_t)arow_s * a.ldA + ca;
    const float* bsrc = Bb + (size_t)brow_s * a.ldB + cb;
    f32x4 va[VEC ? NLA : 1], vb[VEC ? NLB : 1];
    float ra[VEC ? 1 : NLA], rb[VEC ? 1 : NLB];
    auto load_a = [&](int k0, int j) {
        if (VEC) va[j] = *reinterpret_cast<const f32x4*>(asrc + (size_t)(k0 + A_RPR * j) * a.ldA);
        else     ra[j] = asrc[(size_t)(k0 + A_RPR * j) * a.ldA];
    };
    auto load_b = [&](int k0, int j) {
        if (VEC) vb[j] = *reinterpret_cast<const f32x4*>(bsrc + (size_t)(k0 + B_RPR * j) * a.ldB);
        else     rb[j] = bsrc[(size_t)(k0 + B_RPR * j) * a.ldB];
    };
    auto store_a = [&](int buf, int j) {
        if (VEC) *reinterpret_cast<f32x4*>(&As[buf][arow_s + A_RPR * j][acol_s]) = va[j];
        else     As[buf][arow_s + A_RPR * j][acol_s] = ra[j];
    };
    auto store_b = [&](int buf, int j) {
        if (VEC) *reinterpret_cast<f32x4*>(&Bs[buf][brow_s + B_RPR * j][bcol_s]) = vb[j];
        else     Bs[buf][brow_s + B_RPR * j][bcol_s] = rb[j];
    };
    const int nk = a.C / BK;
#pragma unroll
    for (int j = 0; j < NLA; ++j) load_a(0, j);
#pragma unroll
    for (int j = 0; j < NLB; ++j) load_b(0, j);
#pragma unroll
    for (int j = 0; j < NLA; ++j) store_a(0, j);
#pragma unroll
    for (int j = 0; j < NLB; ++j) store_b(0, j);
#pragma unroll
    for (int j = 0; j < NLA; ++j) load_a(BK, j);
#pragma unroll
    for (int j = 0; j < NLB; ++j) load_b(BK, j);
    __syncthreads();

    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.0f;
    const float* arow = &As[0][lrow][wm * 64 + lcol];
    const float* brow = &Bs[0][lrow][wn * 64 + lcol];
    for (int s = 0; s < nk; ++s) {
        const int cur = s & 1;
        const float* ap = arow + cur * (BK * BMA);
        const float* bp = brow + cur * (BK * BN);
        const int k2 = (s + 2 < nk ? s + 2 : nk - 1) * BK;      // past the end: re-load the last step (never consumed)
        float af[2][4][2], bf[2][4][2];
        auto read_chunk = [&](int c, int slot) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = c * 4 + e;
#pragma unroll
                for (int i = 0; i < 2; ++i) af[slot][e][i] = ap[2 * kk * BMA + i * 32];
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[slot][e][j] = bp[2 * kk * BN + j * 32];
            }
        };
        read_chunk(0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c + 1 < 4) read_chunk(c + 1, (c + 1) & 1);
            // the registers hold K step s+1: stored into the other buffer and re-loaded with step s+2 right behind the store
            if (c == 0) {
#pragma unroll
                for (int j = 0; j < NLA; ++j) store_a(cur ^ 1, j);
#pragma unroll
                for (int j = 0; j < NLA; ++j) load_a(k2, j);
            } else if (c == 1) {
#pragma unroll
                for (int j = 0; j < NLB; ++j) store_b(cur ^ 1, j);
#pragma unroll
                for (int j = 0; j < NLB; ++j) load_b(k2, j);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c & 1][e][i], bf[c & 1][e][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (s + 1 == nk || (a.kch && (s + 1) % a.kch == 0)) mnn_close_chunk(tot, acc);
        __syncthreads();
    }
    if (a.maskB) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gj = j0 + (wn * 2 + j) * 32 + lcol;
            const float mk = gj < a.nB ? a.maskB[(size_t)pair * a.strideMask + gj] : 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[i][j][r] *= mk;
        }
    }
    mnn_tile_epilogue<WA>(tot, a, &As[0][0][0], reinterpret_cast<int*>(&Bs[0][0][0]), i0, j0, ta, tb, rowPartVal, rowPartIdx, colPartVal,
                          colPartIdx);
