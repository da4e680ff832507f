// ransac.hip -- RANSAC over 4-point DLT homographies (utils/outil.py:68-164).
//
// The reference drives the loop from the host in chunks of 100 hypotheses: 16 device->host copies, a CPU
// LAPACK SVD, one host->device copy and >= 2 synchronising reads per chunk (utils/outil.py:73,84,86,
// 143-150).  Here the whole search is four asynchronous launches with no host round trip:
//   pack     matches -> (x1,y1,x2,y2) float4 + z2, so scoring issues one 16-byte load per match
//   dlt      one hypothesis per lane: duplicate test (:122-133), float64 Householder DLT (dlt.h,
//            LAPACK-sign-exact), float32 cast, det(H) > 1e-6 gate with torch.det's LU order (:108,113)
//   count    one hypothesis per wavefront: lanes stride over the matches, reprojection error in the
//            reference's float32 operation order (k-ordered fma chain for Y.H^T as sgemm does, IEEE
//            divide, separate squares / add / sqrt), __ballot + popcount for the inlier tally (:97-100,110-113)
//   select   chunk-of-100 zero-abort (:140-146), first maximum over the filtered order (:143-160), inlier
//            mask of the winner (:162-163)
// Every kernel takes one RansacArgs block by value; ransac_pair() is the one place that says where pair b's data lives.
// This TU is compiled with -ffp-contract=off so that only the fmaf calls written below fuse.
#include "common.h"
#include "dlt.h"
#include <math.h>

namespace {

constexpr int CHUNK = 100;         // nbMaxIter, utils/outil.py:136
constexpr int MAX_CHUNKS = 8192;   // LDS table in select kernel -> N <= 819200 hypotheses

// One search: a batch of pairs (rfx_ransac_h4_batched: narr = the match counts on the device, every per-pair array `cap` matches /
// N hypotheses apart) or a single pair (narr == nullptr: n from the host, cap = 0, pair 0).
struct RansacArgs {
    const float* m1; const float* m2;   // (cap,3) matches per pair; the direct DLT form: X, Y (N,4,3)
    const int64_t* samples;             // (N,4) per pair; nullptr = the direct form
    const int32_t* narr; int n;
    int cap, N;
    float tol;
    int filter_dup;
    char* ws;                           // per pair, wsStride bytes apart: P (cap float4), Z (cap f32), H (N,9 f32), flags (N), counts (N i32)
    size_t oP, oZ, oH, oFlags, oCounts, wsStride;
    float* Hout;                        // single pair: the hypotheses go here instead of the workspace's H
    int64_t* counts64;                  // single pair, optional
    float* bestH; uint8_t* inlier; int32_t* result;   // 9 f32, cap (single pair: n) uint8, 4 int32 per pair
};

struct RansacPair {
    const float* m1; const float* m2; const int64_t* samples;
    int n; bool batched;
    float4* P; float* Z; float* H; uint8_t* flags; int* counts;
    float* bestH; uint8_t* inlier; int32_t* result;
};

__device__ __forceinline__ RansacPair ransac_pair(const RansacArgs& a, int b) {
    RansacPair v;
    v.batched = a.narr != nullptr;
    v.n = v.batched ? a.narr[b] : a.n;
    v.m1 = a.m1 + (size_t)b * a.cap * 3; v.m2 = a.m2 + (size_t)b * a.cap * 3;
    v.samples = a.samples ? a.samples + (size_t)b * a.N * 4 : nullptr;
    char* w = a.ws + b * a.wsStride;
    v.P = reinterpret_cast<float4*>(w + a.oP);
    v.Z = reinterpret_cast<float*>(w + a.oZ);
    v.H = a.Hout ? a.Hout : reinterpret_cast<float*>(w + a.oH);
    v.flags = reinterpret_cast<uint8_t*>(w + a.oFlags);
    v.counts = reinterpret_cast<int*>(w + a.oCounts);
    v.bestH = a.bestH + b * 9; v.inlier = a.inlier + (size_t)b * a.cap; v.result = a.result + b * 4;
    return v;
}

// The block for N hypotheses on pairs of up to n_cap matches: the workspace layout, everything else zero.  The direct DLT form has no
// workspace (N = n_cap = 0: every offset 0); its optional flag array stands in as `ws`.
RansacArgs ransac_args(int N, int n_cap, void* ws) {
    RansacArgs a = {};
    a.N = N;
    a.ws = static_cast<char*>(ws);
    size_t o = 0;
    a.oP = o; o += rfx_al256((size_t)n_cap * 16);
    a.oZ = o; o += rfx_al256((size_t)n_cap * 4);
    a.oH = o; o += rfx_al256((size_t)N * 36);
    a.oFlags = o; o += rfx_al256((size_t)N);
    a.oCounts = o; o += rfx_al256((size_t)N * 4);
    a.wsStride = o;
    return a;
}

__global__ __launch_bounds__(256) void ransac_pack_kernel(RansacArgs a) {
    const RansacPair v = ransac_pair(a, blockIdx.y);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < v.n) {
        float4 p;
        p.x = v.m1[i * 3 + 0]; p.y = v.m1[i * 3 + 1];
        p.z = v.m2[i * 3 + 0]; p.w = v.m2[i * 3 + 1];
        v.P[i] = p;
        v.Z[i] = v.m2[i * 3 + 2];
    }
}

// X,Y given either as gathered samples (N,4,3) [no `samples`] or through indices into the match arrays.
// WANT_RANK: also extract the bidiagonal and run the Sturm count behind flag bit 2 (15 fp64 registers and divisions per
// hypothesis) -- only the callers that read the bit ask for it (the staged "lapack" search, the *_flags entry point,
// rfx_score_hypotheses with a `degenerate` output); the throughput path (rfx_ransac_h4[_batched]) does not pay for it.
template <bool WANT_RANK>
__global__ __launch_bounds__(64) void ransac_dlt_kernel(RansacArgs a) {
    const RansacPair v = ransac_pair(a, blockIdx.y);
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= a.N) return;
    const int n = v.n;
    float src[4][2], tgt[4][2];
    bool dup = false, bad = v.batched && n < 4;   // batched: a pair with fewer than nbPoint matches evaluates nothing
    if (v.samples) {
        int64_t s[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) s[p] = v.samples[(size_t)h * 4 + p];
        dup = (s[0] == s[1]) | (s[0] == s[2]) | (s[0] == s[3]) | (s[1] == s[2]) | (s[1] == s[3]) | (s[2] == s[3]);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int64_t q = s[p];
            if (q < 0) q += n;  // python-style negative index
            if (q < 0 || q >= n) { bad = true; q = 0; }
            src[p][0] = v.m1[q * 3 + 0]; src[p][1] = v.m1[q * 3 + 1];
            tgt[p][0] = v.m2[q * 3 + 0]; tgt[p][1] = v.m2[q * 3 + 1];
        }
    } else {  // m1 = X (N,4,3), m2 = Y (N,4,3)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            src[p][0] = v.m1[((size_t)h * 4 + p) * 3 + 0]; src[p][1] = v.m1[((size_t)h * 4 + p) * 3 + 1];
            tgt[p][0] = v.m2[((size_t)h * 4 + p) * 3 + 0]; tgt[p][1] = v.m2[((size_t)h * 4 + p) * 3 + 1];
        }
    }
    uint8_t fl = 0;  // bit0: evaluated (survives the duplicate filter), bit1: det gate passed, bit2: rank-deficient system
    if (!(a.filter_dup && dup) && !bad) {
        double hv[9], bd[15];
        rfx_dlt4_nullvec(src, tgt, hv, WANT_RANK ? bd : nullptr);
        float hf[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) { hf[j] = (float)hv[j]; v.H[(size_t)h * 9 + j] = hf[j]; }
        fl = 1 | (rfx_det3_lu_f32(hf) > 1e-6f ? 2 : 0);   // torch.det's own LU order (dlt.h)
        if (WANT_RANK) fl |= rfx_bidiag_rank_deficient(bd, RFX_DLT_RANK_REL) ? 4 : 0;
    } else {
#pragma unroll
        for (int j = 0; j < 9; ++j) v.H[(size_t)h * 9 + j] = 0.0f;
    }
    if (v.flags) v.flags[h] = fl;
}

__device__ __forceinline__ float reproj_error(const float4 p, const float z, const float* H) {
    // estimX = Y @ H^T : k-ordered fma chain (what the reference's K=3 sgemm evaluates)
    const float px = fmaf(z, H[2], fmaf(p.w, H[1], __fmul_rn(p.z, H[0])));
    const float py = fmaf(z, H[5], fmaf(p.w, H[4], __fmul_rn(p.z, H[3])));
    const float pz = fmaf(z, H[8], fmaf(p.w, H[7], __fmul_rn(p.z, H[6])));
    const float ex = __fdiv_rn(px, pz), ey = __fdiv_rn(py, pz);
    const float dx = __fsub_rn(p.x, ex), dy = __fsub_rn(p.y, ey);
    const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
    return __fsqrt_rn(d2);
}

__device__ __forceinline__ bool is_inlier(const float4 p, const float z, const float* H, const float tol) {
    return reproj_error(p, z, H) < tol;  // NaN (pz == 0) compares false, as in the reference
}

// outil.Prediction (utils/outil.py:97-100): err[h][m] for every (hypothesis, match) pair
__global__ __launch_bounds__(256) void prediction_kernel(const float* __restrict__ m1, const float* __restrict__ m2, int n,
                                                         const float* __restrict__ Hs, int N, float* __restrict__ err) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    const int h = blockIdx.y;
    if (m >= n) return;
    float H[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) H[j] = Hs[(size_t)h * 9 + j];
    float4 p;
    p.x = m1[m * 3 + 0]; p.y = m1[m * 3 + 1]; p.z = m2[m * 3 + 0]; p.w = m2[m * 3 + 1];
    err[(size_t)h * n + m] = reproj_error(p, m2[m * 3 + 2], H);
}

// one hypothesis per wavefront, 4 wavefronts per workgroup
__global__ __launch_bounds__(256) void ransac_count_kernel(RansacArgs a) {
    const RansacPair v = ransac_pair(a, blockIdx.y);
    const int lane = threadIdx.x & 63;
    const int h = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (h >= a.N) return;
    const int n = v.n;
    const uint8_t fl = v.flags[h];
    int cnt = 0;
    if (fl & 1) {
        float H[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) H[j] = v.H[(size_t)h * 9 + j];  // wave-uniform -> scalar loads
        for (int m0 = 0; m0 < n; m0 += 64) {  // wave-uniform trip count (the ballot needs every lane)
            const int m = m0 + lane;
            bool in = false;
            if (m < n) in = is_inlier(v.P[m], v.Z[m], H, a.tol);
            cnt += __popcll(__ballot(in));
        }
        if (!(fl & 2)) cnt = 0;  // counts * (det > 1e-6)
    }
    if (lane == 0) {
        v.counts[h] = (fl & 1) ? cnt : -1;
        if (a.counts64) a.counts64[h] = cnt;
    }
}

__global__ __launch_bounds__(1024) void ransac_select_kernel(RansacArgs a) {
    const RansacPair v = ransac_pair(a, blockIdx.x);
    const int n = v.n, N = a.N;
    const bool too_few = v.batched && n < 4;
    __shared__ int chunkmax[MAX_CHUNKS];
    __shared__ unsigned long long bestkey;
    __shared__ int s_status;
    const int t = threadIdx.x;
    for (int c = t; c < MAX_CHUNKS; c += 1024) chunkmax[c] = 0;
    if (t == 0) { bestkey = 0ull; s_status = 0; }
    RfxOrderedCompact oc = rfx_ordered_compact_begin();
    // rank of every surviving hypothesis in the filtered order, per-chunk maxima, global first maximum
    for (int s = 0; s < N; s += 1024) {
        const int h = s + t;
        const bool keep = h < N && (v.flags[h] & 1);
        const int rank = oc.place(keep);
        if (keep) {
            const int c = v.counts[h];
            atomicMax(&chunkmax[rank / CHUNK], c);
            // larger count wins; equal counts: smaller index wins
            const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)(0xffffffffu - (unsigned)h);
            atomicMax(&bestkey, key);
        }
    }
    __syncthreads();   // the last trip's maxima, before any thread reads them
    const int nUnique = oc.total();
    const int nFull = nUnique / CHUNK;
    bool ab = false;
    for (int c = t; c < nFull; c += 1024) ab |= (chunkmax[c] == 0);
    if (ab) s_status = 1;  // benign race: all writers store 1
    __syncthreads();
    const unsigned long long key = bestkey;
    const int bestCnt = (int)(key >> 32);
    const int bestIdx = (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
    int status = s_status;
    if (status == 0 && (nUnique == 0 || bestCnt == 0)) status = 2;
    if (too_few) status = 3;
    if (t == 0) {
        v.result[0] = status;
        v.result[1] = status == 0 ? bestCnt : 0;
        v.result[2] = status == 0 ? bestIdx : -1;
        v.result[3] = nUnique;
    }
    const int nout = v.batched ? a.cap : n;   // batched: the padding rows of the mask are defined (0) too
    if (status != 0) {
        for (int m = t; m < nout; m += 1024) v.inlier[m] = 0;
        if (t < 9) v.bestH[t] = 0.0f;
        return;
    }
    float H[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) H[j] = v.H[(size_t)bestIdx * 9 + j];
    if (t < 9) v.bestH[t] = H[t];
    for (int m = t; m < nout; m += 1024) v.inlier[m] = (m < n && is_inlier(v.P[m], v.Z[m], H, a.tol)) ? 1 : 0;
}

// ---- rank-deficient hypotheses: list them (ascending, per pair), take re-solved homographies back: ONE row per flagged hypothesis,
// all pairs back to back.  idx (batch,N), cnt (batch).
__global__ __launch_bounds__(1024) void ransac_degen_list_kernel(RansacArgs a, int32_t* __restrict__ idx, int32_t* __restrict__ cnt) {
    const int b = blockIdx.x, t = threadIdx.x;
    const uint8_t* flags = ransac_pair(a, b).flags;
    idx += (size_t)b * a.N;
    RfxOrderedCompact oc = rfx_ordered_compact_begin();
    for (int s = 0; s < a.N; s += 1024) {
        const int h = s + t;
        const bool hit = h < a.N && (flags[h] & 5) == 5;       // evaluated AND rank deficient
        const int pos = oc.place(hit);
        if (hit) idx[pos] = h;
    }
    if (t == 0) cnt[b] = oc.total();
}

// off[b] = rows of the pairs before b (exclusive prefix of cnt), off[batch] = total; written to the device copy the later
// kernels read and to `off_out` (pinned host memory: what the host reads after the event)
__global__ __launch_bounds__(64) void ransac_degen_scan_kernel(const int32_t* __restrict__ cnt, int batch, int32_t* __restrict__ off,
                                                               int32_t* __restrict__ off_out) {
    if (threadIdx.x != 0) return;
    int acc = 0;
    for (int b = 0; b < batch; ++b) { off[b] = acc; if (off_out) off_out[b] = acc; acc += cnt[b]; }
    off[batch] = acc;
    if (off_out) off_out[batch] = acc;
}

// row off[b]+k = the 4 source points (x, y) then the 4 target points (x, y) of pair b's k-th flagged sample: X[:, :, :2] | Y[:, :, :2]
// of outil.Homography's arguments (utils/outil.py:68-71), 64 bytes, straight into pinned host memory
__global__ __launch_bounds__(256) void ransac_degen_gather_kernel(RansacArgs a, const int32_t* __restrict__ idx,
                                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                                                                  float4* __restrict__ xy, int row_cap) {
    const int b = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt[b] || k >= a.N) return;
    const int row = off[b] + k;
    if (row >= row_cap) return;
    const int h = idx[(size_t)b * a.N + k];
    const RansacPair v = ransac_pair(a, b);
    const int n = v.n;
    float c[16];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        int64_t q = v.samples[(size_t)h * 4 + p];
        if (q < 0) q += n;                                   // python-style negative index (as in the DLT kernel)
        if (q < 0 || q >= n) q = 0;
        c[2 * p] = v.m1[q * 3 + 0]; c[2 * p + 1] = v.m1[q * 3 + 1];
        c[8 + 2 * p] = v.m2[q * 3 + 0]; c[8 + 2 * p + 1] = v.m2[q * 3 + 1];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) xy[(size_t)row * 4 + j] = make_float4(c[4 * j], c[4 * j + 1], c[4 * j + 2], c[4 * j + 3]);
}

__global__ __launch_bounds__(256) void ransac_patch_compact_kernel(RansacArgs a, const int32_t* __restrict__ idx,
                                                                const int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                                                                const float* __restrict__ Hp, int row_cap) {
    const int b = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt[b] || k >= a.N) return;
    const int row = off[b] + k;
    if (row >= row_cap) return;
    const int h = idx[(size_t)b * a.N + k];
    if (h < 0 || h >= a.N) return;
    const RansacPair v = ransac_pair(a, b);
    float hf[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) { hf[j] = Hp[(size_t)row * 9 + j]; v.H[(size_t)h * 9 + j] = hf[j]; }
    v.flags[h] = (v.flags[h] & ~2) | (rfx_det3_lu_f32(hf) > 1e-6f ? 2 : 0);
}

int ransac_dlt(const RansacArgs& a, int batch, bool want_rank, hipStream_t st) {
    const dim3 grid((a.N + 63) / 64, batch);
    if (want_rank) hipLaunchKernelGGL(ransac_dlt_kernel<true>, grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL(ransac_dlt_kernel<false>, grid, dim3(64), 0, st, a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

// pack + DLT: the packed matches, the hypotheses and their flags into the workspace
int ransac_hypotheses(const RansacArgs& a, int batch, bool want_rank, hipStream_t st) {
    const int nmax = a.narr ? a.cap : a.n;
    hipLaunchKernelGGL(ransac_pack_kernel, dim3((nmax + 255) / 256, batch), dim3(256), 0, st, a);
    RFX_LAUNCH_CHECK();
    return ransac_dlt(a, batch, want_rank, st);
}

int ransac_count(const RansacArgs& a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(ransac_count_kernel, dim3((a.N + 3) / 4, batch), dim3(256), 0, st, a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

int ransac_select(const RansacArgs& a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(ransac_select_kernel, dim3(batch), dim3(1024), 0, st, a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

// outil.Homography on gathered samples (no `samples`, no workspace); degenerate (optional) receives the flags of every system
int ransac_dlt_direct(const float* X, const float* Y, int N, float* Hout, uint8_t* degenerate, void* stream) {
    if (!X || !Y || !Hout || N <= 0) return RFX_E_ARG;
    RansacArgs a = ransac_args(0, 0, degenerate);
    a.m1 = X; a.m2 = Y; a.N = N; a.Hout = Hout;
    return ransac_dlt(a, 1, degenerate != nullptr, rfx_stream(stream));
}

}  // namespace

extern "C" int rfx_dlt4_homography(const float* X, const float* Y, int N, float* Hout, void* stream) {
    return ransac_dlt_direct(X, Y, N, Hout, nullptr, stream);
}

// outil.Homography with the rank flag per system (degenerate (N) uint8: bit 2 = rank deficient, see dlt.h)
extern "C" int rfx_dlt4_homography_flags(const float* X, const float* Y, int N, float* Hout, uint8_t* degenerate, void* stream) {
    if (!degenerate) return RFX_E_ARG;
    return ransac_dlt_direct(X, Y, N, Hout, degenerate, stream);
}

extern "C" int rfx_prediction_f32(const float* match1, const float* match2, int n, const float* Hs, int N, float* err,
                                  void* stream) {
    if (!match1 || !match2 || !Hs || !err || n <= 0 || N <= 0 || N > 65535) return RFX_E_ARG;
    hipLaunchKernelGGL(prediction_kernel, dim3((n + 255) / 256, N), dim3(256), 0, rfx_stream(stream), match1, match2, n,
                       Hs, N, err);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" size_t rfx_ransac_ws_bytes(int n, int N) {
    if (N <= 0 || n <= 0) return 0;
    return ransac_args(N, n, nullptr).wsStride;
}

extern "C" int rfx_score_hypotheses(const float* match1, const float* match2, int n, const int64_t* samples, int N,
                                    float tol, float* Hout, int64_t* counts, uint8_t* flags_out, void* ws, void* stream) {
    if (!match1 || !match2 || !samples || !Hout || !counts || !ws || n <= 0 || N <= 0) return RFX_E_ARG;
    RansacArgs a = ransac_args(N, n, ws);
    a.m1 = match1; a.m2 = match2; a.samples = samples; a.n = n; a.tol = tol;
    a.Hout = Hout; a.counts64 = counts;
    hipStream_t st = rfx_stream(stream);
    int rc = ransac_hypotheses(a, 1, flags_out != nullptr, st);
    if (rc == RFX_OK) rc = ransac_count(a, 1, st);
    if (rc != RFX_OK || !flags_out) return rc;
    // the per-hypothesis flags of the SAME DLT pass (bit 2 = rank-deficient system): no second solve for the caller that patches
    hipError_t e = hipMemcpyAsync(flags_out, a.ws + a.oFlags, (size_t)N, hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? RFX_OK : (int)e;
}

extern "C" int rfx_ransac_h4(const float* match1, const float* match2, int n, const int64_t* samples, int N, float tol,
                             float* bestH, uint8_t* inlier, int32_t* result, void* ws, void* stream) {
    if (!match1 || !match2 || !samples || !bestH || !inlier || !result || !ws || n <= 0 || N <= 0) return RFX_E_ARG;
    if ((N + CHUNK - 1) / CHUNK > MAX_CHUNKS) return RFX_E_LIMIT;
    RansacArgs a = ransac_args(N, n, ws);
    a.m1 = match1; a.m2 = match2; a.samples = samples; a.n = n; a.tol = tol; a.filter_dup = 1;
    a.bestH = bestH; a.inlier = inlier; a.result = result;
    hipStream_t st = rfx_stream(stream);
    int rc = ransac_hypotheses(a, 1, false, st);
    if (rc == RFX_OK) rc = ransac_count(a, 1, st);
    if (rc == RFX_OK) rc = ransac_select(a, 1, st);
    return rc;
}

// ---- batched RANSAC: every pair of a batch in ONE launch chain (pack, DLT, count, select), match counts read from a
// device array.  Same kernels, same arithmetic per pair as rfx_ransac_h4.
extern "C" size_t rfx_ransac_batched_ws_bytes(int cap, int N, int batch) {
    if (N <= 0 || cap <= 0 || batch <= 0) return 0;
    return ransac_args(N, cap, nullptr).wsStride * (size_t)batch;
}

// stages: 1 = pack + DLT (hypotheses and their flags into the workspace), 2 = count + select; 3 = both
extern "C" int rfx_ransac_h4_batched_stage(const float* match1, const float* match2, const int32_t* n, int cap,
                                           const int64_t* samples, int N, float tol, float* bestH, uint8_t* inlier,
                                           int32_t* result, void* ws, int batch, int stages, void* stream) {
    if (!match1 || !match2 || !n || !samples || !bestH || !inlier || !result || !ws || cap <= 0 || N <= 0 || batch <= 0 ||
        stages < 1 || stages > 3)
        return RFX_E_ARG;
    if ((N + CHUNK - 1) / CHUNK > MAX_CHUNKS || batch > 65535) return RFX_E_LIMIT;
    RansacArgs a = ransac_args(N, cap, ws);
    a.m1 = match1; a.m2 = match2; a.samples = samples; a.narr = n; a.cap = cap; a.tol = tol; a.filter_dup = 1;
    a.bestH = bestH; a.inlier = inlier; a.result = result;
    hipStream_t st = rfx_stream(stream);
    int rc = RFX_OK;
    // the rank flag is read between the stages of the staged ("lapack") search only: stages == 3 is the throughput path
    if (stages & 1) rc = ransac_hypotheses(a, batch, stages == 1, st);
    if (rc == RFX_OK && (stages & 2)) rc = ransac_count(a, batch, st);
    if (rc == RFX_OK && (stages & 2)) rc = ransac_select(a, batch, st);
    return rc;
}

extern "C" int rfx_ransac_h4_batched(const float* match1, const float* match2, const int32_t* n, int cap,
                                     const int64_t* samples, int N, float tol, float* bestH, uint8_t* inlier,
                                     int32_t* result, void* ws, int batch, void* stream) {
    return rfx_ransac_h4_batched_stage(match1, match2, n, cap, samples, N, tol, bestH, inlier, result, ws, batch, 3, stream);
}

extern "C" int rfx_ransac_degenerate_gather(const void* ws, const float* match1, const float* match2, const int32_t* n, int cap,
                                            const int64_t* samples, int N, int batch, int32_t* idx, int32_t* count, int32_t* off,
                                            int32_t* off_host, float* xy_rows, int row_cap, void* stream) {
    if (!ws || !match1 || !match2 || !n || !samples || !idx || !count || !off || !xy_rows || cap <= 0 || N <= 0 || batch <= 0 ||
        row_cap <= 0)
        return RFX_E_ARG;
    if (batch > 65535) return RFX_E_LIMIT;
    RansacArgs a = ransac_args(N, cap, const_cast<void*>(ws));
    a.m1 = match1; a.m2 = match2; a.samples = samples; a.narr = n; a.cap = cap;
    hipStream_t st = rfx_stream(stream);
    hipLaunchKernelGGL(ransac_degen_list_kernel, dim3(batch), dim3(1024), 0, st, a, idx, count);
    RFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_degen_scan_kernel, dim3(1), dim3(64), 0, st, count, batch, off, off_host);
    RFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_degen_gather_kernel, dim3((N + 255) / 256, batch), dim3(256), 0, st, a, idx, count, off,
                       reinterpret_cast<float4*>(xy_rows), row_cap);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_ransac_patch_h_rows(void* ws, int cap, int N, int batch, const int32_t* idx, const int32_t* count,
                                       const int32_t* off, const float* H_rows, int row_cap, void* stream) {
    if (!ws || !idx || !count || !off || !H_rows || cap <= 0 || N <= 0 || batch <= 0 || row_cap <= 0) return RFX_E_ARG;
    if (batch > 65535) return RFX_E_LIMIT;
    RansacArgs a = ransac_args(N, cap, ws);
    a.cap = cap;
    hipLaunchKernelGGL(ransac_patch_compact_kernel, dim3((N + 255) / 256, batch), dim3(256), 0, rfx_stream(stream), a, idx, count, off,
                       H_rows, row_cap);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

// match1[b,i] = (xa[idx1[b,i]], ya[idx1[b,i]], 1), match2[b,i] = (xb[idx2[b,i]], yb[idx2[b,i]], 1) for i < n[b], zeros after:
// the match lists of quick_start/coarseAlignFeatMatch.py:150-155 for a whole batch in one launch.
namespace {
// The body both gather kernels run; every pointer is already moved to pair b (xa / ya / xb / yb to its cell coordinates).
__device__ __forceinline__ void gather_matches_body(const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2, int n, int cap,
                                                    const float* __restrict__ xa, const float* __restrict__ ya,
                                                    const float* __restrict__ xb, const float* __restrict__ yb,
                                                    float* __restrict__ m1, float* __restrict__ m2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    const size_t o = (size_t)i * 3;
    if (i < n) {
        const int64_t a = idx1[i], t = idx2[i];
        m1[o] = xa[a]; m1[o + 1] = ya[a]; m1[o + 2] = 1.0f;
        m2[o] = xb[t]; m2[o + 1] = yb[t]; m2[o + 2] = 1.0f;
    } else {
        m1[o] = m1[o + 1] = m1[o + 2] = 0.0f;
        m2[o] = m2[o + 1] = m2[o + 2] = 0.0f;
    }
}

// blockIdx.y = pair b.  Ragged batch (offA): pair b's cell coordinates are its own slice of the packed tables, xa/ya + offA[b] and
// xb/yb + offB[b]; dense batch (offA == nullptr): every pair reads the same tables.
__global__ __launch_bounds__(256) void gather_matches_kernel(const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2,
                                                             const int32_t* __restrict__ narr, int cap,
                                                             const float* __restrict__ xa, const float* __restrict__ ya,
                                                             const float* __restrict__ xb, const float* __restrict__ yb,
                                                             float* __restrict__ m1, float* __restrict__ m2) {
    const size_t b = blockIdx.y;
    gather_matches_body(idx1 + b * cap, idx2 + b * cap, narr[b], cap, xa, ya, xb, yb, m1 + b * cap * 3, m2 + b * cap * 3);
}

__global__ __launch_bounds__(256) void gather_matches_ragged_kernel(const int64_t* __restrict__ idx1, const int64_t* __restrict__ idx2,
                                                                    const int32_t* __restrict__ narr, int cap,
                                                                    const float* __restrict__ xa, const float* __restrict__ ya,
                                                                    const long long* __restrict__ offA, const float* __restrict__ xb,
                                                                    const float* __restrict__ yb, const long long* __restrict__ offB,
                                                                    float* __restrict__ m1, float* __restrict__ m2) {
    const size_t b = blockIdx.y;
    gather_matches_body(idx1 + b * cap, idx2 + b * cap, narr[b], cap, xa + offA[b], ya + offA[b], xb + offB[b], yb + offB[b],
                        m1 + b * cap * 3, m2 + b * cap * 3);
}
}  // namespace

extern "C" int rfx_gather_matches_ragged_f32(const int64_t* idx1, const int64_t* idx2, const int32_t* n, int cap, const float* xa,
                                             const float* ya, const long long* offA, const float* xb, const float* yb,
                                             const long long* offB, float* match1, float* match2, int batch, void* stream) {
    if (!idx1 || !idx2 || !n || !xa || !ya || !offA || !xb || !yb || !offB || !match1 || !match2 || cap <= 0 || batch <= 0)
        return RFX_E_ARG;
    if (batch > 65535) return RFX_E_LIMIT;
    hipLaunchKernelGGL(gather_matches_ragged_kernel, dim3((cap + 255) / 256, batch), dim3(256), 0, rfx_stream(stream), idx1, idx2,
                       n, cap, xa, ya, offA, xb, yb, offB, match1, match2);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_gather_matches_f32(const int64_t* idx1, const int64_t* idx2, const int32_t* n, int cap, const float* xa,
                                      const float* ya, const float* xb, const float* yb, float* match1, float* match2,
                                      int batch, void* stream) {
    if (!idx1 || !idx2 || !n || !xa || !ya || !xb || !yb || !match1 || !match2 || cap <= 0 || batch <= 0) return RFX_E_ARG;
    if (batch > 65535) return RFX_E_LIMIT;
    hipLaunchKernelGGL(gather_matches_kernel, dim3((cap + 255) / 256, batch), dim3(256), 0, rfx_stream(stream), idx1, idx2, n,
                       cap, xa, ya, xb, yb, match1, match2);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
