// corr.hip -- 7x7 local correlation volume (CorrNeigh, model/model.py:129-160):
//     out[n, i*7+j, r, c] = sum_ch x[n,ch,r,c] * y[n,ch,r+i-3,c+j-3]        (y zero outside the image)
//
// The reference runs 49 separate multiply+reduce kernels that each re-read x and y (49x the minimal
// traffic).  Here every x/y element is fetched from HBM once per tile (+ halo), staged in LDS by the
// LDS-DMA path (global_load_lds_dwordx4: no VGPR round trip, zero fill by pointing out-of-image
// lanes at a 16-byte zero block) and all 49 taps of 4 horizontally adjacent pixels are accumulated in
// registers (4 px x 28 / 21 taps per lane), so one LDS float feeds ~2.3 FMAs and the kernel sits on the
// fp32 VALU, next to the HBM roofline (algorithmic intensity 11 FLOP/B).
//
// Tile = TR rows x 16*NCB columns per workgroup.  The tile shape decides the HBM traffic: the y operand needs a
// 3-pixel halo, so a 16x16 tile fetches (22x24)/(16x16) = 2.06x its y pixels, while a tile that spans the whole
// image width (NCB = W/16: the column halo lies outside the image and is zero-filled for free) only pays the
// row halo, 22/16 -- and the rows above/below the image cost nothing either.  At the 60x80 maps of a 480x640 pair
// the full-width 16-row tile moves 1.14x the algorithmic bytes instead of 1.37x.
//
// One wavefront = 16 rows x 16 columns x one group of window rows (taps i = 0..3: 112 accumulators / lane, or
// i = 4..6: 84); lane -> (tc = lane>>4: 4-pixel column group, r = lane&15: row).  LDS per channel: y halo tile
// [TR+6][16*NCB+8] floats (row stride 64*NCB+32 B = 6 mod 16 quads: the 16-lane ds_read_b128 service groups hit 16
// distinct 16-B slots -> conflict free for every NCB), x tile [TR][16*NCB].  Channels are streamed CK at a time
// through an NS-deep LDS ring: one raw s_barrier per chunk and a COUNTED s_waitcnt vmcnt, so the DMA of the next
// NS-2 chunks stays in flight across the barrier while chunk s is on the VALU (a __syncthreads() would drain it
// with vmcnt(0)).  Channel sums are accumulated in channel order with fmaf (deterministic); the translation unit
// is built with -fno-slp-vectorize: the SLP vectoriser pairs the FMAs into v_pk_fma_f32 over register pairs that
// are misaligned for half the taps and pays ~0.5 v_mov per FMA to re-pack them, while a plain v_fmac_f32 issues at
// the full fp32 rate on gfx950's SIMD-32.
//
// Requires W % 4 == 0 for the 16-byte DMA path; other widths use the plain fallback kernel below.
#include "common.h"
#include "group.h"
#include <hip/hip_ext.h>
#include <vector>

namespace {

// ---- kernel-duration capture (rfx_corr_timing / rfx_corr_timing_collect, round 6) ------------------------------------------------
// bench.py prices this kernel against the HBM roofline by its DURATION.  An event pair recorded around a launch brackets the
// command processor's work on both sides as well (~18 us next to a 150 us kernel: round 5's BENCH line read 0.515 where rocprofv3's
// kernel duration gave 0.577).  hipExtLaunchKernelGGL attaches a start and a stop event to the dispatch packet itself -- the
// timestamps rocprofv3 reads -- so, while a host thread has the capture on, its correlation launches carry a library-owned event pair.
thread_local bool t_timing = false;
thread_local std::vector<std::pair<hipEvent_t, hipEvent_t>> t_events;

template <class K, class... Args>
inline void corr_launch(K kernel, dim3 grid, dim3 block, hipStream_t st, Args... args) {
    if (t_timing) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            hipExtLaunchKernelGGL(kernel, grid, block, 0, st, e0, e1, 0, args...);
            t_events.emplace_back(e0, e1);
            return;
        }
        if (e0) (void)hipEventDestroy(e0);
    }
    hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
}

constexpr int TC = 16;           // columns per wavefront

// Kernel configuration: tile TR x 16*NCB columns, in one of two families (each with and without the BIDIR epilogue):
//   plain: 2 groups of window rows (4+3; 3 waves / SIMD, 168 VGPRs), ring of 3, compiler-scheduled LDS reads, out-of-image lanes
//          fetch the 16-byte zero block, full TR-row tiles;
//   TUNED: 3 groups (3+2+2; 4 waves / SIMD, 128 VGPRs), ring of 4, LDS reads hand-pipelined one (channel, window row) step ahead
//          (corr7_steps), halo / padding slots zeroed ONCE with the DMA lanes that would fetch zeros masked off, x rows padded to
//          the y row stride (conflict-free ds_read_b128 of x), s_setprio 1 for the waves of the 3-row group, H split into equal
//          row tiles, and at NCB == 5 the SIMD-balanced wave map below.
template <int TR_, int NCB_, bool TUNED_, bool BIDIR_>
struct Cfg {
    static constexpr int TR = TR_, NCB = NCB_;
    static constexpr bool TUNED = TUNED_;
    static constexpr bool BIDIR = BIDIR_;   // also write corr(y, x): the same products at mirrored taps / shifted pixels
    static constexpr int CK = 2;                               // channels per chunk
    static constexpr int NS = TUNED ? 4 : 3;                   // LDS ring depth
    static constexpr int NG = TUNED ? 3 : 2;                   // groups of window rows (one wavefront per 16x16 block and group)
    static constexpr int NW = TR / 16 * NCB * NG;              // waves per workgroup: strips x column blocks x tap-row groups
    static constexpr int YR = TR + 6;                          // halo rows
    static constexpr int YQ = 4 * NCB + 2;                     // float4 per halo row (cols c0-4 .. c0+16*NCB+3)
    static constexpr int XQ = TUNED ? 4 * NCB + 2 : 4 * NCB;   // float4 slots per x row (4*NCB used)
    static constexpr int Y_SLOTS = CK * YR * YQ;               // float4 slots of the y halo tile
    static constexpr int Y_PIECES = (Y_SLOTS + 63) / 64;
    static constexpr int X_SLOTS = CK * TR * XQ;
    static constexpr int X_PIECES = (X_SLOTS + 63) / 64;
    static constexpr int PPW = (Y_PIECES + X_PIECES + NW - 1) / NW;   // DMA pieces per wave per chunk (padded)
    static constexpr int N_PIECES = PPW * NW;                  // incl. padding pieces (dump area, never read)
    static constexpr int BUF_SLOTS = N_PIECES * 64;
    // window rows of group g: [row_begin(g), row_begin(g+1))  -- 2 groups: 4+3, 3 groups: 3+2+2
    static constexpr int row_begin(int g) { return NG == 2 ? (g == 0 ? 0 : g == 1 ? 4 : 7) : (g == 0 ? 0 : g == 1 ? 3 : g == 2 ? 5 : 7); }
    static constexpr int WAVES_PER_SIMD = NG == 2 ? 3 : 4;     // register budget: 168 / 128 VGPRs
    // wave -> (16x16 block, tap group).  The hardware deals a workgroup's waves to the 4 SIMDs cyclically (w, w+4, w+8 ..
    // share one), and the groups are unequal (3 vs 2 vs 2 window rows), so the plain map w -> (w / NG, w % NG) of the 15-wave
    // tile gives one SIMD {H,L,L,H} (560 FMAs per chunk against an average of 490); the balanced map puts 3 x {H,L,L,L} + {H,H,L}
    // on the SIMDs (worst: 504).  The 12- and 9-wave tiles get one wave of each group per SIMD from the plain map.
    static constexpr bool BALANCED = TUNED && NCB == 5;
    static constexpr int wave_group(int w) {
        if (!BALANCED) return w % NG;
        return (w <= 3 || w == 7) ? 0 : ((w <= 6 || w == 8 || w == 9) ? 1 : 2);
    }
    static constexpr int wave_block(int w) {           // rank of w among the waves of its group
        if (!BALANCED) return w / NG;
        int r = 0;
        for (int v = 0; v < w; ++v) r += wave_group(v) == wave_group(w);
        return r;
    }
    static_assert(!TUNED || TR == 16, "the tuned family has 16-row tiles");
    static_assert(NW * 64 <= 1024, "workgroup too large");
    static_assert((NS - 2) * PPW <= 15, "vmcnt immediate out of range (wait_vm)");
    static_assert((size_t)NS * BUF_SLOTS * 16 <= 160 * 1024, "LDS ring exceeds 160 KiB");
};

__device__ __attribute__((aligned(16))) float rfx_zero16[4] = {0.f, 0.f, 0.f, 0.f};

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// ---- LDS reads of the compute loop as inline assembly -------------------------------------------------------------
// hipcc (ROCm 7.2) classifies global_load_lds as a FLAT access that may touch LDS and, while one is pending -- always, in
// this kernel -- waits for EVERY outstanding ds_read with s_waitcnt lgkmcnt(0): a read issued one step ahead of its use
// is then drained together with the newest ones and the prefetch distance collapses to zero.  The reads and their
// COUNTED waits are therefore written by hand: ds_read_b128 with a compile-time byte offset, and s_waitcnt lgkmcnt(K)
// carrying the registers it makes valid as in/out operands so that no use can be scheduled above it.
template <int OFF>
__device__ __forceinline__ void lds_read128(f32x4& d, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
template <int K>
__device__ __forceinline__ void lds_wait(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(K));
}

// One (channel, window row) step of a chunk, ST = 0 .. CK*NI-1, recursively unrolled (the offsets must be immediates).  The reads
// of step ST+1 are issued before the FMAs of step ST.
template <class G, int I0, int I1, int ST>
__device__ __forceinline__ void corr7_steps(f32x4 (&wq)[G::CK * (I1 - I0)][3], f32x4 (&xq)[G::CK], float (&acc)[4][(I1 - I0) * 7],
                                            unsigned ya, unsigned xa) {
    constexpr int NI = I1 - I0, NSTEP = G::CK * NI;
    constexpr int YROW = G::YQ * 16, YCH = G::YR * G::YQ * 16, XCH = G::TR * G::XQ * 16;
    if constexpr (ST == 0) {          // pipeline fill: step 0 (+ the x quad of channel 0)
        lds_read128<0>(xq[0], xa);
        lds_read128<I0 * YROW>(wq[0][0], ya);
        lds_read128<I0 * YROW + 16>(wq[0][1], ya);
        lds_read128<I0 * YROW + 32>(wq[0][2], ya);
    }
    constexpr int S2 = ST + 1;        // the step whose reads are issued now
    if constexpr (S2 < NSTEP) {
        constexpr int o = (S2 / NI) * YCH + (I0 + S2 % NI) * YROW;
        if constexpr (S2 % NI == 0) lds_read128<(S2 / NI) * XCH>(xq[S2 / NI], xa);
        lds_read128<o>(wq[S2][0], ya); lds_read128<o + 16>(wq[S2][1], ya); lds_read128<o + 32>(wq[S2][2], ya);
    }
    // reads issued after those of step ST: the 3 of step ST+1, + 1 where that step opens a channel
    constexpr int NEWER = S2 < NSTEP ? 3 + (S2 % NI == 0 ? 1 : 0) : 0;
    constexpr int ch = ST / NI, r = ST % NI;
    lds_wait<NEWER>(wq[ST][0], wq[ST][1], wq[ST][2], xq[ch]);
    const f32x4 w0 = wq[ST][0], w1 = wq[ST][1], w2 = wq[ST][2], xv = xq[ch];
    // element e = d+j+1 of the 12-float window, picked straight out of the three quads (an intermediate float[12] makes
    // the optimiser re-load the window from the wq array with overlapping 48-byte loads, which pins wq in scratch)
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int e = d + j + 1;
            const float yv = e < 4 ? w0[e & 3] : (e < 8 ? w1[e & 3] : w2[e & 3]);
            float& a = acc[d][r * 7 + j];
            a = fmaf(xv[d], yv, a);
        }
    if constexpr (ST + 1 < NSTEP) corr7_steps<G, I0, I1, ST + 1>(wq, xq, acc, ya, xa);
}

// s_waitcnt vmcnt(n) for a wave-uniform n (the immediate must be a constant): n = DMA instructions of this wave that may
// stay in flight = younger chunks x pieces this wave issues per chunk.
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
#define RFX_VM(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
        RFX_VM(0) RFX_VM(1) RFX_VM(2) RFX_VM(3) RFX_VM(4) RFX_VM(5) RFX_VM(6) RFX_VM(7) RFX_VM(8) RFX_VM(9) RFX_VM(10) RFX_VM(11)
        RFX_VM(12) RFX_VM(13) RFX_VM(14) RFX_VM(15)
#undef RFX_VM
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;   // conservative
    }
}

// One wavefront = one 16-row strip x one 16-column block of the tile x one group of window rows I0..I1-1 (4 px x 7 x
// (I1-I0) accumulators per lane).  Splitting the 49 taps over NG wavefronts divides the register footprint (3 or 4
// instead of 2 wavefronts per SIMD); all groups read the same LDS tile, so the DMA traffic is unchanged.
template <class G, int I0, int I1>
__device__ __forceinline__ void corr7_strip(f32x4* smem, const float* xn, const float* yn, const int* off, int wave, int amask,
                                            int strip, int cb, int lane, int nchunks, size_t HW,
                                            float* __restrict__ out, float* __restrict__ out21, int n, int row0, int c0, int H,
                                            int W, int trv) {
    constexpr int NI = I1 - I0, NS = G::NS, CK = G::CK, TR = G::TR;
    auto issue = [&](int chunk, int buf) {
        const size_t cbase = (size_t)chunk * CK * HW;
#pragma unroll
        for (int i = 0; i < G::PPW; ++i) {
            const int pi = wave + G::NW * i;
            const float* base = (pi < G::Y_PIECES ? yn : xn) + cbase;
            if constexpr (G::TUNED) {
                // slots outside the image were zeroed once: their lanes are masked off (no fetch, no LDS write) and a piece
                // without any image data is not issued at all (amask / npieces are wave-uniform: the vmcnt arithmetic below
                // counts THIS wave's issues).  No zero block, hence no scalar load in the loop: an SMEM op in flight would
                // make the counted lgkmcnt waits of the LDS-read pipeline unsafe (scalar loads return out of order).
                if ((amask >> i) & 1)
                    if (off[i] >= 0)
                        __builtin_amdgcn_global_load_lds((gptr_t)(base + off[i]), (lptr_t)(smem + buf * G::BUF_SLOTS + pi * 64), 16, 0, 0);
            } else {
                const float* src = off[i] >= 0 ? base + off[i] : rfx_zero16;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + buf * G::BUF_SLOTS + pi * 64), 16, 0, 0);
            }
        }
    };
    const int npieces = G::TUNED ? __builtin_popcount((unsigned)amask) : G::PPW;   // DMA instructions per chunk of this wave
    float acc[4][NI * 7];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int q = 0; q < NI * 7; ++q) acc[d][q] = 0.f;
    const int tc = lane >> 4;
    const int tr = strip * 16 + (lane & 15);
    const int yoff = tr * G::YQ + cb * 4 + tc;        // slot of (row tr, this lane's first window quad) in a channel's y tile
    const int xoff = tr * G::XQ + cb * 4 + tc;
    const unsigned lds_base = (unsigned)(uintptr_t)(lptr_t)smem;   // LDS byte address of the ring

    // prologue: chunks 0 .. NS-2 in flight
#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
        if (p < nchunks) issue(p, p);
    int buf = 0;
    for (int s = 0; s < nchunks; ++s) {
        // chunk s must have landed; the (up to NS-2) younger chunks of this wave may stay in flight across the barrier
        const int younger = nchunks - 1 - s < NS - 2 ? nchunks - 1 - s : NS - 2;
        wait_vm(younger * npieces);
        __builtin_amdgcn_s_barrier();  // all waves: chunk s visible, and everyone is done reading buffer (s-1)%NS
        if (s + NS - 1 < nchunks) issue(s + NS - 1, buf == 0 ? NS - 1 : buf - 1);  // (s+NS-1)%NS == (s-1)%NS
        if constexpr (G::TUNED) {
            // hand-pipelined LDS reads (see lds_read128): byte addresses of this lane's first window quad / x quad
            const unsigned ya = lds_base + (unsigned)(buf * G::BUF_SLOTS + yoff) * 16u;
            const unsigned xa = lds_base + (unsigned)(buf * G::BUF_SLOTS + G::Y_PIECES * 64 + xoff) * 16u;
            f32x4 wq[CK * NI][3];
            f32x4 xq[CK];
            corr7_steps<G, I0, I1, 0>(wq, xq, acc, ya, xa);
        } else {
            const f32x4* yb = smem + buf * G::BUF_SLOTS + yoff;
            const f32x4* xb = smem + buf * G::BUF_SLOTS + G::Y_PIECES * 64 + xoff;
#pragma unroll
            for (int ch = 0; ch < CK; ++ch) {
                const f32x4 xv = xb[ch * (TR * G::XQ)];
#pragma unroll
                for (int i = I0; i < I1; ++i) {
                    const f32x4* yrow = yb + ch * (G::YR * G::YQ) + i * G::YQ;
                    const f32x4 w0 = yrow[0], w1 = yrow[1], w2 = yrow[2];
                    const float yw[12] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};
#pragma unroll
                    for (int d = 0; d < 4; ++d)
#pragma unroll
                        for (int j = 0; j < 7; ++j)
                            acc[d][(i - I0) * 7 + j] = fmaf(xv[d], yw[d + j + 1], acc[d][(i - I0) * 7 + j]);
                }
            }
        }
        buf = buf == NS - 1 ? 0 : buf + 1;
    }
    const int gr = row0 + tr, gc = c0 + cb * TC + 4 * tc;
    if (tr < trv && gr < H && gc < W) {
        float* o = out + (size_t)n * 49 * HW + (size_t)gr * W + gc;
#pragma unroll
        for (int q = 0; q < NI * 7; ++q) {
            f32x4 v = {acc[0][q], acc[1][q], acc[2][q], acc[3][q]};
            *reinterpret_cast<f32x4*>(o + (size_t)(I0 * 7 + q) * HW) = v;
        }
        if constexpr (G::BIDIR) {
            // corr(y, x)[(6-i)*7 + (6-j), r+i-3, c+j-3] = corr(x, y)[i*7 + j, r, c]: the SAME channel-ordered sum (products
            // commute bit for bit), so the reverse direction of a pair is this lane's accumulators stored once more at the
            // mirrored tap and the shifted pixel.  A destination whose source pixel lies outside the image is a zero of
            // the reverse volume (its window tap falls into the padding, model/model.py:135,143): the lane that OWNS that
            // destination pixel writes the zero, so every element of out21 is written exactly once.
            float* o21 = out21 + (size_t)n * 49 * HW;
#pragma unroll
            for (int q = 0; q < NI * 7; ++q) {
                const int i = I0 + q / 7, j = q % 7;
                float* pl = o21 + (size_t)((6 - i) * 7 + (6 - j)) * HW;
                const int dr = gr + i - 3;
                if ((unsigned)dr < (unsigned)H) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int dc = gc + d + j - 3;
                        if ((unsigned)dc < (unsigned)W) pl[(size_t)dr * W + dc] = acc[d][q];
                    }
                }
                const int sr = gr - (i - 3);                    // source row of this lane's own pixels in plane (6-i, 6-j)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int sc = gc + d - (j - 3);
                    if ((unsigned)sr >= (unsigned)H || (unsigned)sc >= (unsigned)W) pl[(size_t)gr * W + gc + d] = 0.f;
                }
            }
        }
    }
}

// Argument block of the DMA kernels.  The body is a typed device function of (arguments, the problem's own block index): the single
// launch and the grouped launch (group.h) both call it.
struct CorrArgs {
    const float* x; const float* y; float* out; float* out21;
    int N, C, H, W, tilesR, tilesC, trv;
};

template <class G>
__device__ __forceinline__ void corr7_dma_body(const CorrArgs& a, const unsigned bx, const unsigned) {
    const float* __restrict__ x = a.x;
    const float* __restrict__ y = a.y;
    float* __restrict__ out = a.out;
    float* __restrict__ out21 = a.out21;
    const int N = a.N, C = a.C, H = a.H, W = a.W, tilesR = a.tilesR, tilesC = a.tilesC, trv = a.trv;
    constexpr int TR = G::TR, NCB = G::NCB, NG = G::NG;
    __shared__ __attribute__((aligned(16))) f32x4 smem[G::NS * G::BUF_SLOTS];

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tpi = tilesR * tilesC;
    const int nwg = N * tpi;
    int bid = (int)bx;
    {   // XCD-aware bijective remap: all tiles of one image on one XCD (halo re-reads hit that L2).  xcd_remap() (common.h) written
        // out: through the helper the six 16-column-tile instances compile to different set-up code.  nwg is the PROBLEM's own
        // workgroup count, also in a grouped launch (whose gridDim.x is the largest problem's): the map stays a bijection of
        // [0, nwg); there it is a locality hint only (workgroups of the other problems share the XCD round-robin)
        const int q = nwg / 8, r = nwg % 8, xcd = bid % 8, j = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    }
    const int n = bid / tpi;
    const int tile = bid - n * tpi;
    // trv <= TR rows of the tile are real (H is split into equal tiles: 60 rows = 4 x 15, so that every workgroup streams
    // the same amount of data; the last lanes of a strip idle instead of one workgroup in four being 25% short)
    const int row0 = (tile / tilesC) * trv, c0 = (tile % tilesC) * (TC * NCB);
    const size_t HW = (size_t)H * W;
    const float* xn = x + (size_t)n * C * HW;
    const float* yn = y + (size_t)n * C * HW;

    // per-lane source offsets of the PPW DMA pieces this wave issues per chunk; -1 = 16-byte zero block / zeroed slot
    int off[G::PPW];
    int amask = 0;
#pragma unroll
    for (int i = 0; i < G::PPW; ++i) {
        // wave is never negative.  The select is kept on purpose: without it the set-up code of the two 16x16-tile instances comes
        // out one instruction (a v_bfe_i32) shorter than in the build the recorded measurements were taken on
        const int pi = wave < 0 ? G::N_PIECES : wave + G::NW * i;
        int o = -1;
        if (pi < G::Y_PIECES) {
            const int s = pi * 64 + lane;
            if (s < G::Y_SLOTS) {
                const int ch = s / (G::YR * G::YQ), rem = s - ch * (G::YR * G::YQ);
                const int rr = rem / G::YQ, q = rem - rr * G::YQ;
                const int gr = row0 + rr - 3, gc = c0 - 4 + 4 * q;
                if (rr < trv + 6 && (unsigned)gr < (unsigned)H && (unsigned)gc < (unsigned)W) o = (int)(ch * HW) + gr * W + gc;
            }
        } else if (pi < G::Y_PIECES + G::X_PIECES) {
            const int s = (pi - G::Y_PIECES) * 64 + lane;
            if (s < G::X_SLOTS) {
                const int ch = s / (TR * G::XQ), rem = s - ch * (TR * G::XQ);
                const int rr = rem / G::XQ, q = rem - rr * G::XQ;
                const int gr = row0 + rr, gc = c0 + 4 * q;
                if (q < 4 * NCB && rr < trv && gr < H && gc < W) o = (int)(ch * HW) + gr * W + gc;
            }
        }
        if (G::TUNED && __ballot(o >= 0) != 0ull) amask |= 1 << i;     // wave-uniform: this piece carries image data
        off[i] = o;
    }
    if (G::TUNED) {
        // zero the out-of-image / padding slots of every ring buffer ONCE: the DMA never writes them again
#pragma unroll
        for (int i = 0; i < G::PPW; ++i)
            if (off[i] < 0) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b = 0; b < G::NS; ++b) smem[b * G::BUF_SLOTS + (wave + G::NW * i) * 64 + lane] = z;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the raw s_barrier of the main loop does not wait for ds_write
    }
    int sc = wave / NG, grp = wave - sc * NG;
    if constexpr (G::BALANCED) {
        constexpr unsigned long long gmap = []() { unsigned long long m = 0; for (int w = 0; w < G::NW; ++w) m |= (unsigned long long)G::wave_group(w) << (2 * w); return m; }();
        constexpr unsigned long long bmap = []() { unsigned long long m = 0; for (int w = 0; w < G::NW; ++w) m |= (unsigned long long)G::wave_block(w) << (4 * w); return m; }();
        grp = (int)((gmap >> (2 * wave)) & 3);
        sc = (int)((bmap >> (4 * wave)) & 15);
    }
    const int strip = sc / NCB, cb = sc - strip * NCB;
    const int nch = C / G::CK;
#define RFX_STRIP(g) corr7_strip<G, G::row_begin(g), G::row_begin(g + 1)>(smem, xn, yn, off, wave, amask, strip, cb, lane, nch, HW, out, out21, n, row0, c0, H, W, trv)
    if (G::TUNED && grp == 0) __builtin_amdgcn_s_setprio(1);   // the 3-row group has the most FMAs per chunk: let it win VALU arbitration
    if (grp == 0) RFX_STRIP(0);
    else if (grp == 1) RFX_STRIP(1);
    if constexpr (NG > 2) { if (grp == 2) RFX_STRIP(2); }
#undef RFX_STRIP
}

// grouped (group.h): one bucket per tile variant -- a problem keeps the variant auto_variant() gives it alone
template <class G> using CorrDma = RfxFamily<CorrArgs, corr7_dma_body<G>, G::NW * 64, G::WAVES_PER_SIMD>;

template <class G>
__global__ __launch_bounds__((CorrDma<G>::BLOCK), (CorrDma<G>::min_waves())) void corr7_dma_kernel(CorrArgs a) {
    corr7_dma_body<G>(a, blockIdx.x, gridDim.x);
}

template <class G>
static int launch_corr(const float* x, const float* y, float* out, float* out21, int N, int C, int H, int W, hipStream_t st) {
    const int tilesR = (H + G::TR - 1) / G::TR;
    const int tilesC = (W + TC * G::NCB - 1) / (TC * G::NCB);
    const int trv = G::TUNED ? (H + tilesR - 1) / tilesR : G::TR;  // equal row tiles (60 = 4 x 15) or full TR-row tiles
    const CorrArgs a = {x, y, out, out21, N, C, H, W, tilesR, tilesC, trv};
    const unsigned nwg = (unsigned)(N * tilesR * tilesC);
    if (rfx_group_recording()) return CorrDma<G>::record(a, nwg);   // never with t_timing: entry points
    corr_launch((corr7_dma_kernel<G>), dim3(nwg), dim3(CorrDma<G>::BLOCK), st, a);
    return RFX_OK;
}

// Plain fallback for widths that are not a multiple of 4 (never hit by the reference's /8 feature maps of
// x16-rounded images, kept so the entry point is total): one thread per output pixel.
struct CorrPlainArgs { const float* x; const float* y; float* out; long long NP; int C, H, W; };

// (grid-stride by the problem's own grid gx: in a grouped launch gridDim.x is the largest problem's)
__device__ __forceinline__ void corr7_plain_body(const CorrPlainArgs& a, const unsigned bx, const unsigned gx) {
    const float* __restrict__ x = a.x;
    const float* __restrict__ y = a.y;
    float* __restrict__ out = a.out;
    const long long NP = a.NP;
    const int C = a.C, H = a.H, W = a.W;
    const size_t HW = (size_t)H * W;
    for (long long p = (long long)bx * blockDim.x + threadIdx.x; p < NP;
         p += (long long)gx * blockDim.x) {
        const long long n = p / HW;
        const int px = (int)(p - n * HW);
        const int r = px / W, c = px - r * W;
        const float* xn = x + (size_t)n * C * HW;
        const float* yn = y + (size_t)n * C * HW;
        for (int i = 0; i < 7; ++i)
            for (int j = 0; j < 7; ++j) {
                const int yr = r + i - 3, yc = c + j - 3;
                float s = 0.f;
                if ((unsigned)yr < (unsigned)H && (unsigned)yc < (unsigned)W)
                    for (int ch = 0; ch < C; ++ch)
                        s = fmaf(xn[ch * HW + px], yn[ch * HW + (size_t)yr * W + yc], s);
                out[(size_t)n * 49 * HW + (size_t)(i * 7 + j) * HW + px] = s;
            }
    }
}

using CorrPlain = RfxFamily<CorrPlainArgs, corr7_plain_body, 256>;
__global__ __launch_bounds__(CorrPlain::BLOCK) void corr7_plain_kernel(CorrPlainArgs a) { corr7_plain_body(a, blockIdx.x, gridDim.x); }

// Variant table (rfx_corr_neigh_variant_f32 / RFX_CORR_VARIANT; 0 = automatic): the six tile shapes auto_variant() returns.
// All are bit-identical; every other number is RFX_E_ARG.  BIDIR: the form that also writes corr(y, x) to out21.
//   1: 64x16   2: 32x16   3: 16x16      plain 16-column tiles
//   5: 16x80   8: 16x64   7: 16x48      tuned tiles (15 / 12 / 9 waves)
template <bool BIDIR>
static int launch_variant(int v, const float* x, const float* y, float* out, float* out21, int N, int C, int H, int W,
                          hipStream_t st) {
    switch (v) {
        case 1: return launch_corr<Cfg<64, 1, false, BIDIR>>(x, y, out, out21, N, C, H, W, st);
        case 2: return launch_corr<Cfg<32, 1, false, BIDIR>>(x, y, out, out21, N, C, H, W, st);
        case 3: return launch_corr<Cfg<16, 1, false, BIDIR>>(x, y, out, out21, N, C, H, W, st);
        case 5: return launch_corr<Cfg<16, 5, true, BIDIR>>(x, y, out, out21, N, C, H, W, st);
        case 7: return launch_corr<Cfg<16, 3, true, BIDIR>>(x, y, out, out21, N, C, H, W, st);
        case 8: return launch_corr<Cfg<16, 4, true, BIDIR>>(x, y, out, out21, N, C, H, W, st);
        default: return RFX_E_ARG;
    }
}

// Tile shape by traffic first, parallelism second.  A tile spanning the image width has no column halo and its row-halo
// re-reads hit the XCD's L2 (measured: 1.00x the algorithmic bytes leave L2 at 60x80, against 1.37x for 16x16 tiles); it is
// taken when the launch still gives most CUs a workgroup.  Otherwise 16-column tiles, as tall as the workgroup count allows
// (>= 1024 workgroups).
static int auto_variant(int N, int H, int W) {
    const long long tc = (W + TC - 1) / TC;
    const long long r16 = (H + 15) / 16;
    if (W > 32 && (long long)N * r16 * ((W + 79) / 80) >= 128) {
        // tuned kernel: the tile width (80 / 64 / 48 columns) that pads the map width least; ties -> the widest
        int best = 5, best_w = 1 << 30;
        for (int ncb = 5; ncb >= 3; --ncb) {
            const int padded = (W + 16 * ncb - 1) / (16 * ncb) * (16 * ncb);
            if (padded < best_w) { best_w = padded; best = ncb; }
        }
        return best == 5 ? 5 : (best == 4 ? 8 : 7);
    }
    const long long b64 = (long long)N * ((H + 63) / 64) * tc, b32 = (long long)N * ((H + 31) / 32) * tc;
    return b64 >= 1024 ? 1 : (b32 >= 1024 ? 2 : 3);
}

static bool dma_ok(const void* a, const void* b, const void* c, const void* d, int C, int W) {
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return W % 4 == 0 && C % 2 == 0 && al(a) && al(b) && al(c) && al(d);
}

}  // namespace

extern "C" int rfx_corr_neigh_variant_f32(const float* x, const float* y, float* out, int N, int C, int H, int W, int K,
                                          int variant, void* stream) {
    if (!x || !y || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return RFX_E_ARG;
    if (K != 7) return RFX_E_ARG;
    if (rfx_group_recording() && t_timing) return RFX_E_ARG;        // the dispatch-event capture belongs to single launches
    if ((long long)C * H * W > 0x7fffffffLL) return RFX_E_LIMIT;
    hipStream_t st = rfx_stream(stream);
    if (dma_ok(x, y, out, nullptr, C, W)) {
        if ((long long)N * ((H + 15) / 16) * ((W + TC - 1) / TC) > 0x7fffffffLL) return RFX_E_LIMIT;
        const int rc = launch_variant<false>(variant == 0 ? auto_variant(N, H, W) : variant, x, y, out, nullptr, N, C, H, W, st);
        if (rc != RFX_OK) return rc;
    } else {
        const long long NP = (long long)N * H * W;
        long long g = (NP + CorrPlain::BLOCK - 1) / CorrPlain::BLOCK;
        if (g > 8192) g = 8192;
        const CorrPlainArgs a = {x, y, out, NP, C, H, W};
        return CorrPlain::launch(corr7_plain_kernel, a, (unsigned)g, st);
    }
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_corr_neigh_f32(const float* x, const float* y, float* out, int N, int C, int H, int W, int K,
                                  void* stream) {
    return rfx_corr_neigh_variant_f32(x, y, out, N, C, H, W, K, 0, stream);
}

extern "C" int rfx_corr_neigh_bidir_f32(const float* x, const float* y, float* out_xy, float* out_yx, int N, int C, int H, int W,
                                        int K, void* stream) {
    if (!x || !y || !out_xy || !out_yx || N <= 0 || C <= 0 || H <= 0 || W <= 0) return RFX_E_ARG;
    if (K != 7) return RFX_E_ARG;
    if (rfx_group_recording() && t_timing) return RFX_E_ARG;        // the dispatch-event capture belongs to single launches
    if ((long long)C * H * W > 0x7fffffffLL) return RFX_E_LIMIT;
    if (!dma_ok(x, y, out_xy, out_yx, C, W)) return RFX_E_ARG;       // the host mirrors pad the width to a multiple of 4
    if ((long long)N * ((H + 15) / 16) * ((W + TC - 1) / TC) > 0x7fffffffLL) return RFX_E_LIMIT;
    const int rc = launch_variant<true>(auto_variant(N, H, W), x, y, out_xy, out_yx, N, C, H, W, rfx_stream(stream));
    if (rc != RFX_OK) return rc;
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_corr_timing(int enable) {
    const int prev = t_timing ? 1 : 0;
    t_timing = enable != 0;
    return prev;
}

extern "C" int rfx_corr_timing_collect(float* us_out, int cap) {
    int n = 0;
    for (auto& ev : t_events) {
        float ms = -1.0f;
        if (hipEventSynchronize(ev.second) == hipSuccess) (void)hipEventElapsedTime(&ms, ev.first, ev.second);
        if (us_out && n < cap) us_out[n] = ms * 1e3f;
        ++n;
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    t_events.clear();
    return n;
}
