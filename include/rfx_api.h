/*
 * rfx_api.h -- C ABI of librfx.so: the MI355X (gfx950 / CDNA4) kernels behind the RANSAC-Flow
 * coarse-to-fine alignment hot path.
 *
 * The reference (XiSHEN0220/RANSAC-Flow) is pure Python on PyTorch: it has no FFI of its own, its
 * "native" layer is the set of ATen/cuDNN/LAPACK ops its hot path issues.
 * Each entry point below replaces one of those op groups; the reference call site it stands in for
 * is cited as file:line relative to the reference root.  The Python drop-in modules
 * (ransac-flow_amd/dropin/{outil,model,coarseAlignFeatMatch}.py) keep the reference's Python
 * surface and bind these symbols through ctypes (see INTEGRATION.md for the stub a maintainer adds).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless the name ends in
 *     _host; all tensors are dense, row-major, float32 ("f32") unless stated; NCHW images.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream), allocates nothing, and never throws: the return value is 0 on success, a negative
 *     RFX_E_* code for a bad argument, or a positive hipError_t from the launch.
 *   - workspaces are caller-owned; rfx_*_ws_bytes() reports the size needed.
 */
#ifndef RFX_API_H
#define RFX_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFX_OK 0
#define RFX_E_ARG (-1)     /* null pointer / non-positive size / unsupported geometry */
#define RFX_E_LIMIT (-2)   /* size above a compiled-in limit */

#define RFX_ACT_NONE 0
#define RFX_ACT_RELU 1
#define RFX_ACT_SIGMOID 2

/* library / build identification; returns a static string "rfx <version> gfx950". */
const char* rfx_version(void);

/* ABI revision of this header: bumped whenever an entry point changes its signature or its operand layout (round 2:
 * rfx_compose_flow_f32 gained Hc/Wc, 3x3/s1/p1 geometries moved to rfx_conv3x3_f32's packed weights; round 3: multi-homography
 * round kernels, two-direction correlation, grouped launches; round 4: rfx_draw_samples_i64 keyed by pair id; 11: the ragged-batch
 * entry points -- mutual NN, feature norm scatter, match gather -- for batches of pairs of different sizes; 12: the ragged forms of the
 * multi-homography round kernels, rfx_filter_matches_ragged_f32 and rfx_multih_accept_ragged_f32; 13:
 * rfx_conv1x1_split_tile_channels; 14: the ragged forms of the KITTI round kernels, rfx_remove_small_cc_ragged_f32 and
 * rfx_multih_accept_ragged_d2_f32; 15: rfx_conv1x1_expand64_f32 and rfx_conv1x1_expand64_dual_f32; 16:
 * rfx_group_stats, and the fine-stage entry points record inside a group; 17: rfx_ransac_degenerate_list and rfx_ransac_patch_h
 * removed, superseded since 9 by rfx_ransac_degenerate_gather / rfx_ransac_patch_h_rows; rfx_keep_mask_ragged_f32 was ADDED under 17,
 * and so were rfx_epe_ws_bytes, rfx_epe_homography_f32, rfx_epe_flow_f32, rfx_assemble_records_f32, rfx_assemble_kitti_records_f32
 * and rfx_kitti_scores_records_f32, then rfx_records_keypoints_f32 and rfx_pck_tally_f64, then
 * rfx_warp_records_u8 and rfx_warp_flow_u8: no existing entry point moved, and a binding that knows
 * a new name refuses a library without it).  A binding
 * compares rfx_abi_version() with the RFX_ABI_VERSION it was written against and refuses a mismatch. */
#define RFX_ABI_VERSION 17
int rfx_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Grouped launches: ONE launch per kernel instance for the same layer of several INDEPENDENT problems of different
 * sizes.  A single pair runs the trunk on 8 images of 8 sizes (7 pyramid levels + the target,
 * quick_start/coarseAlignFeatMatch.py:92-125): layer by layer that is 8 launches of 2-150 workgroups on 256 CUs, bound
 * by one workgroup lifetime per layer AND level.  Between rfx_group_begin() and rfx_group_end() the convolution entry
 * points (rfx_conv2d_f32, rfx_conv3x3_f32, rfx_conv3x3_conv1x1_f32, rfx_stem_conv7x7_maxpool_f32) and, since ABI 16, the
 * fine-stage entry points (rfx_stem_conv3x3_maxblur_f32, rfx_blurpool2d_f32, rfx_l2norm_nchw_f32, rfx_flow_head_f32,
 * rfx_resize_bilinear_f32, rfx_corr_neigh_f32 / _variant_f32 / _bidir_f32, rfx_warp_grid_f32, rfx_grid_sample_f32,
 * rfx_compose_flow_f32: PredFlowMask over several shape groups as one chain of grouped launches) validate and RECORD
 * their launch instead of issuing it; rfx_group_end(stream) issues, per kernel instance, one launch whose blockIdx.y
 * selects the problem (up to 8 per launch).  The device code of a problem is the single launch's, so results are
 * bit-identical.  Recording is per host thread, groups do not nest, every other entry point launches immediately;
 * the caller keeps all operands alive until rfx_group_end and records only mutually independent calls.
 * rfx_group_abort() drops a recording without launching.  The kernel instances of one group that remain distinct run
 * concurrently on two library-owned side streams forked from / joined to `stream`; rfx_group_side_streams(0) turns that off
 * for the calling host thread (returns the previous setting) -- a caller that already runs several grouped chains on streams
 * of its own (rfx/pipeline.py: the images of a single pair as two chains) wants each chain serial on its stream.
 * A recorded call may not read what another call of the SAME group writes: all launches are issued at rfx_group_end.
 * rfx_group_stats: cumulative counts of the calling host thread -- rfx_group_end calls and the kernel launches they issued
 * (one per kernel instance and chunk of 8 problems); either pointer may be NULL.
 * ------------------------------------------------------------------------------------------ */
int rfx_group_begin(void);
int rfx_group_end(void* stream);
int rfx_group_abort(void);
int rfx_group_side_streams(int enable);
int rfx_group_stats(long long* groups, long long* launches);

/* ------------------------------------------------------------------------------------------
 * Convolution family (ResNet-50 conv1..layer3 trunk: model/resnet50.py:68-104,112-169 as used by
 * quick_start/coarseAlignFeatMatch.py:34-52,106,124; FeatureExtractor model/model.py:59-125;
 * NetFlowCoarse / NetMatchability convs model/model.py:210-226,289-305).
 *
 * rfx_conv2d_f32: implicit-GEMM convolution on the fp32 MFMA (v_mfma_f32_32x32x2_f32), NCHW,
 * groups=1, dilation=1, with a fused per-output-channel affine (eval-mode BatchNorm folded to
 * scale/shift), optional residual add and activation:
 *     out[n,m,oh,ow] = act( scale[m] * sum_{c,kh,kw} in[n,c,oh*s-p+kh,ow*s-p+kw] * w[m,c,kh,kw]
 *                           + shift[m] + residual[n,m,oh,ow] )
 * wT    : packed weights [Kpad][Mpad], wT[k*Mpad+m] = w[m,c,kh,kw] with k=(c*KH+kh)*KW+kw,
 *         Kpad = roundup(Cin*KH*KW,32), Mpad = roundup(Cout,128), zero padded.
 * ktab  : int32[Kpad], (c<<8)|(kh<<4)|kw for k < K and -1 for the padding rows, stored per block of 32
 *         consecutive k as [16 even k | 16 odd k].
 * scale/shift may be NULL (treated as 1 / 0); residual may be NULL.
 * ------------------------------------------------------------------------------------------ */
int rfx_conv2d_f32(const float* in, const float* wT, const int32_t* ktab, const float* scale,
                   const float* shift, const float* residual, float* out, int N, int Cin, int Hin,
                   int Win, int Cout, int KH, int KW, int stride, int pad, int act, void* stream);

/* Which tile configuration rfx_conv2d_f32 launches for an output of (N, Cout, Hout, Wout):
 * 0 = 128x128 (kernel conv2d_mfma_kernel<2,2>), 1 = 64x128 (<1,2>), 2 = 64x64 (<1,1>).  Lets a profiler-side
 * caller attribute algorithmic FLOPs to the kernel instance rocprofv3 reports. */
int rfx_conv2d_tile_variant(int N, int Cout, int Hout, int Wout);

/* Kernel-instance id a convolution of this geometry runs as, for a profiler-side caller and for the host mirrors' routing.  THE bit
 * layout of every *_kernel_id of this header (the library writes it in one place, csrc/conv_dispatch.h ConvInstance::id()):
 *   bits 8-13 name the kernel family, none of them set = the implicit-GEMM kernel of rfx_conv2d_f32:
 *     (none)  conv2d_mfma_kernel<TM, TN, ONE, WS, VECB>: bits 0-1 = tile variant (rfx_conv2d_tile_variant), bit 2 = 1x1 specialisation,
 *             bit 3 = wave-specialised form (4 MFMA + 4 loader wavefronts), bit 4 = 16-byte pixel-side loads (1x1, stride 1)
 *     bit 10  conv1x1_kmajor_kernel<TM, VEC, KCH>, the k-major 1x1 / stride 1 kernel rfx_conv2d_f32 runs for Cin % 32 == 0, Cin >= 64
 *             (bit 2 is set with it): bit 0 = 64-channel tiles (TM = 1), bit 4 = VEC
 *     bit 5   conv3x3_direct_kernel<TM, PT_C, false, TN, RAG, KCH>, the direct 3x3 / stride 1 / pad 1 kernel (Cin >= 8), served by
 *             rfx_conv3x3_f32 (the host mirrors call it then; rfx_conv2d_f32 itself never runs it): bit 0 = 64-channel tiles (TM = 1),
 *             bits 6-7 = output patch shape (0: 8x16, 1: 16x8, 2: 32x4 -- the one that pads the stacked N x (H x W) maps least),
 *             bit 11 = 256-pixel (16x16) patches, TN = 4 (Cout <= 64 on launches of >= 1024 such patches: twice the pixels per staged
 *             weight image), bit 12 = the instance with a ragged last K step, RAG (Cin % 8 != 0)
 *     bit 13  conv3x3_s2_kernel<TM, KCH>, the direct 3x3 / STRIDE 2 / pad 1 kernel (Cin % 8 == 0), served by rfx_conv3x3_s2_f32: ResNet-50
 *             layer2.0 / layer3.0 conv2 (model/resnet50.py:75), the first convolution of FeatureExtractor layer2 / layer3
 *             (model/model.py:86-95): bit 0 = 64-channel tiles (TM = 1)
 *     bit 9   conv3x3_direct_kernel<TM, PT_C, true, 2, false, KCH>, the fused Bottleneck tail rfx_conv3x3_conv1x1_f32: bit 0 = 64-channel
 *             mid tile (TM = 1), bits 6-7 = output patch shape as for bit 5
 *     (bit 8: the fused stems; bits 15-16: the split-arithmetic kernels -- ids of the Python profiler, not of the library)
 *   bit 14 = chunked accumulation (KCH > 0): on layers whose K is long -- 3x3 / stride 1 with K = 9 Cin >= 2048 and the 3x3 of a Bottleneck
 *     tail (KCH = 4: a chunk = 4 K steps = 288 products), 3x3 / stride 2 with K >= 1152 (KCH = 4), 1x1 / stride 1 with K >= 512 (KCH = 8:
 *     256 products, 64-channel tiles at every launch size) -- the accumulators are added to a running total at the end of every chunk and
 *     restarted, the K-blocked sum of the reference's CPU kernels (MKL sgemm / oneDNN) instead of ONE fma chain over K: 2.7-3.8x less
 *     round-off against float64 at K = 2304 / 4608.  On those 3x3 layers rfx_conv2d_f32 (its implicit-GEMM kernel: a chain) and
 *     rfx_conv3x3_f32 therefore differ in the last bits -- everywhere else they are bit-identical; the long-K 1x1 layers run chunked
 *     through rfx_conv2d_f32 itself.  RFX_C3_CHUNK=0 / RFX_C1_CHUNK=0: chains (A/B runs).
 * The answer is the one the launch functions act on at the moment of the call: between rfx_group_begin and rfx_group_end it is the
 * instance a recorded launch takes.  A query sees no pointer: bit 4 is cleared at launch for an input that is not 16-byte aligned. */
int rfx_conv2d_kernel_id(int N, int Cin, int Cout, int KH, int KW, int stride, int pad, int Hout, int Wout);

/* 3x3 / stride 1 / pad 1 convolution, Cin >= 8 (a Cin that is not a multiple of 8 -- the 49-channel correlation volume in
 * front of the heads -- takes ceil(Cin/8) K steps, the packed weights carrying zero rows for the missing channels) (ResNet Bottleneck conv2 at stride 1, model/resnet50.py:75; the
 * FeatureExtractor BasicBlocks, model/model.py:32-35; the NetFlowCoarse / NetMatchability stacks, model/model.py:170-181):
 * the direct kernel that stages the raw input patch in LDS.  Same epilogue and the same result, bit for bit, as
 * rfx_conv2d_f32; the weights come packed in the kernel's own LDS order so that staging is a straight copy:
 *     wP[mt][s][h][m][kk] = w[mt*128 + m, c, kh, kw]   with k = (c*3 + kh)*3 + kw = s*72 + 2*kk + h,
 *     mt < roundup(Cout,128)/128, s < ceil(Cin/8), h < 2, m < 128, kk < 36; zero for mt*128 + m >= Cout and for c >= Cin; 16-byte aligned.
 * k_chunk (ABI 8): 0 = the library's rule (chunked accumulation, bit 14 of rfx_conv2d_kernel_id, for K = 9 Cin >= 2048); 4 = close a chunk every 4 K
 * steps (288 products) whatever K is -- what rfx_conv3x3_conv1x1_f32 does in its 3x3 phase since round 5, so that a Bottleneck
 * tail run as two kernels (this one with k_chunk = 4, then the 1x1) equals the fused kernel bit for bit.  Other values: RFX_E_ARG.
 * rfx_conv3x3_kernel_id: the instance this call launches (bits as rfx_conv2d_kernel_id). */
int rfx_conv3x3_f32(const float* in, const float* wP, const float* scale, const float* shift, const float* residual,
                    float* out, int N, int Cin, int H, int W, int Cout, int act, int k_chunk, void* stream);
int rfx_conv3x3_kernel_id(int N, int Cin, int Cout, int H, int W, int k_chunk);
/* The same for stride 2 (pad 1, Cin % 8 == 0): out (N, Cout, (H-1)/2+1, (W-1)/2+1); wP as above.  Bit-identical to
 * rfx_conv2d_f32 on the same geometry for K = 9 Cin < 1152 ONLY: from Cin = 128 on (K >= 1152) this kernel sums in chunks of 288
 * products (conv3x3_s2_kernel<TM, 4>: bit 14 of rfx_conv2d_kernel_id), the implicit-GEMM kernel behind rfx_conv2d_f32 in ONE chain -- the two
 * then differ in the last bit, and so do trunk features when the host mirror is switched to the generic kernel (RFX_CONV_S2=0 /
 * RFX_CONV_DIRECT=0 are A/B switches for experiments, not product settings: they change the sums). */
int rfx_conv3x3_s2_f32(const float* in, const float* wP, const float* scale, const float* shift, const float* residual,
                       float* out, int N, int Cin, int H, int W, int Cout, int act, void* stream);

/* Bottleneck tail (model/resnet50.py:71-79, forward :93-103: conv2 3x3 -> bn2 -> relu -> conv3 1x1 -> bn3 -> += residual
 * -> relu) as ONE kernel: out = act3(bn3(conv1x1(act2(bn2(conv3x3(in))))) + residual).  The workgroup that computed a
 * 128-pixel tile of ALL Cmid channels of the 3x3 convolution keeps it in LDS and multiplies it with the expansion weights,
 * so the Cmid-channel map never goes to HBM.  in (N,Cin,H,W); wP2/scale2/shift2 = weights (packed as for
 * rfx_conv3x3_f32) / folded BN of the 3x3 (stride 1, pad 1, Cin % 8 == 0, Cmid = 64 or 128); scale3 / shift3 of the 1x1 (Cexp % 128 == 0) and its weights in
 * "quad" order wQ3[q][h][m][j] = W3[m][8q + 2j + h] (q < Cmid/8, h < 2, m < Cexp, j < 4; 16-byte aligned): the four MFMA A
 * operands of a lane for four consecutive k-pairs are one 16-byte load, coalesced over the channels;
 * residual (N,Cexp,H,W) or NULL; act2 / act3 = RFX_ACT_NONE or RFX_ACT_RELU.
 * Round 5: the 3x3 phase (K = 9 Cmid = 576 / 1152) closes a chunk every 4 K steps (288 products) into a second accumulator set --
 * the last place the device summed a long K as ONE fma chain while the reference's oneDNN kernels block it.
 * Bit-identical to rfx_conv3x3_f32(k_chunk = 4) followed by the 1x1 through rfx_conv2d_f32.  RFX_C3_TAIL_CHUNK=0: round 4's chain. */
/* Kernel instance of the launch below (bits as rfx_conv2d_kernel_id: bit 9 and its fields). */
int rfx_conv3x3_conv1x1_kernel_id(int N, int H, int W, int Cmid);
int rfx_conv3x3_conv1x1_f32(const float* in, const float* wP2, const float* scale2, const float* shift2, int act2,
                            const float* wQ3, const float* scale3, const float* shift3, const float* residual, int act3,
                            float* out, int N, int Cin, int H, int W, int Cmid, int Cexp, void* stream);

/* nn.MaxPool2d(k, stride, pad) with -inf padding (model/resnet50.py:120: k=3,s=2,p=1;
 * model/model.py:71: k=2,s=1,p=0).  Hout = (Hin+2p-k)/s+1. */
int rfx_maxpool2d_f32(const float* in, float* out, int NC, int Hin, int Win, int k, int stride,
                      int pad, void* stream);

/* Anti-aliased down-sampling (model/downsample.py:12-46, filt_size=3): reflect-pad 1, depthwise
 * [1 2 1]x[1 2 1]/16, stride.  Hout = (Hin-1)/stride+1.  Records inside a group (rfx_group_begin). */
int rfx_blurpool2d_f32(const float* in, float* out, int NC, int Hin, int Win, int stride, void* stream);

/* Fused MaxPool2d(kernel 2, stride 1) + BlurPool(stride): the FeatureExtractor stem `self.maxpool`
 * (model/model.py:71-72).  Hout = (Hin-2)/stride+1.  Bit-identical to the two separate calls. */
int rfx_maxblurpool2d_f32(const float* in, float* out, int NC, int Hin, int Win, int stride, void* stream);

/* The whole FeatureExtractor stem in one kernel (model/model.py:68-72, forward :106-110): conv3x3(3 -> Cout, stride 1,
 * pad 1) + folded BatchNorm + ReLU + MaxPool2d(2, stride 1) + BlurPool(stride 2).  in (N,3,H,W); wT / scale / shift as
 * for rfx_conv2d_f32 (the packed weights of that convolution: K = 27 -> Kpad = 32 rows); out (N,Cout,(H-2)/2+1,(W-2)/2+1).
 * Bit-identical to rfx_conv2d_f32(act = ReLU) followed by rfx_maxblurpool2d_f32(stride 2); the full-resolution
 * Cout-channel map never goes to HBM.  Cout % 32 == 0.  Records inside a group (rfx_group_begin). */
int rfx_stem_conv3x3_maxblur_f32(const float* in, const float* wT, const float* scale, const float* shift, float* out,
                                 int N, int H, int W, int Cout, void* stream);

/* The ResNet-50 stem in one kernel (model/resnet50.py:115-120, forward :157-160): conv7x7(3 -> Cout, stride 2, pad 3) +
 * folded BatchNorm + ReLU + MaxPool2d(3, stride 2, pad 1).  in (N,3,H,W); wT / scale / shift = the packed weights of that
 * convolution (K = 147 -> Kpad = 160 rows); out (N,Cout,Hp,Wp) with Hc = (H-1)/2+1, Hp = (Hc-1)/2+1 (same for W).
 * Bit-identical to rfx_conv2d_f32(act = ReLU) followed by rfx_maxpool2d_f32(3, 2, 1).  Cout % 32 == 0. */
int rfx_stem_conv7x7_maxpool_f32(const float* in, const float* wT, const float* scale, const float* shift, float* out,
                                 int N, int H, int W, int Cout, void* stream);

/* F.normalize(x, p=2, dim=1, eps=1e-12) on NCHW (quick_start/coarseAlignFeatMatch.py:106,124;
 * quick_start/align2images.py:87-88).  `in` is dense; element (n,c,p) of the result goes to
 * out[n*out_batch_stride + c*out_chan_stride + p] (0 = dense defaults C*HW / HW), which lets the coarse
 * aligner write every pyramid scale straight into the concatenated (C, nA) match matrix
 * (quick_start/coarseAlignFeatMatch.py:108,115).  In-place allowed for the dense case.  Records inside a group
 * (rfx_group_begin): the four-wavefront kernel (C % 4 == 0, C >= 32) and the one-wavefront kernel are two kernel instances. */
int rfx_l2norm_nchw_f32(const float* in, float* out, int N, int C, int HW, long long out_batch_stride,
                        long long out_chan_stride, void* stream);
/* (ABI 11) The same norm, sums bit for bit, for the N images of one shape bucket of a ragged batch (quick_start/
 * coarseAlignFeatMatch.py:106,124 per image): image n of in (N,C,HW) goes to out + dst_off[n] with channel stride out_chan_stride
 * (>= HW); dst_off (N) int64 element offsets, e.g. its pair's column offset in the padded (batch,C,ldA) match matrix.  One
 * launch per bucket instead of one per image.  Requires C % 4 == 0 and C >= 32. */
int rfx_l2norm_nchw_scatter_f32(const float* in, float* out, int N, int C, int HW, const long long* dst_off,
                                long long out_chan_stride, void* stream);

/* NetFlowCoarse tail (model/model.py:228-233): softmax over the K*K logits, expectation of the tap
 * offsets; flow[n,0] = sum_q p_q * gx_q / cols * 2, flow[n,1] = sum_q p_q * gy_q / rows * 2 with
 * q = i*K+j, gx_q = j-K/2, gy_q = i-K/2.  logits (N,K*K,rows,cols) -> flow (N,2,rows,cols).  Records inside a group
 * (rfx_group_begin). */
int rfx_flow_head_f32(const float* logits, float* flow, int N, int K, int rows, int cols, void* stream);

/* Bilinear resize of NCHW maps: F.interpolate(mode='bilinear', align_corners=False)
 * (quick_start/align2images.py:92, evaluation/evalHpatch/evaluation.py:37-40) or
 * F.upsample_bilinear (= align_corners=True; model/model.py:234,309).  Records inside a group (rfx_group_begin). */
int rfx_resize_bilinear_f32(const float* in, float* out, int NC, int Hin, int Win, int Hout, int Wout,
                            int align_corners, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image pre-processing on the device (host-side in the reference:
 * quick_start/coarseAlignFeatMatch.py:55-57,80-110).
 * ------------------------------------------------------------------------------------------ */
/* One separable pass of Pillow's fixed-point LANCZOS resampler on uint8 NHWC images (C <= 4).
 * vertical = 0: out (N, outH, outW, C) with out row y filtered from source row y + row_offset (outH + row_offset
 * <= inH); vertical = 1: out (N, outH, inW, C) (outW must equal inW).  bounds: int32 (n_out, 2) = [first source
 * index, tap count] per output coordinate; weights: int32 (n_out, ksize) = round(w * 2^22) (Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc; rfx/lanczos.py computes them).  Integer arithmetic: bit-identical to
 * PIL.Image.resize(resample=LANCZOS) when the two passes are chained as Pillow does. */
int rfx_lanczos_pass_u8(const uint8_t* in, uint8_t* out, int N, int inH, int inW, int outH, int outW, int C,
                        const int32_t* bounds, const int32_t* weights, int ksize, int vertical, int row_offset,
                        void* stream);

/* torchvision ToTensor (+ Normalize): uint8 (N,H,W,3) -> float32 (N,3,H,W).  raw = x/255 (may be NULL),
 * norm = (x/255 - mean[c]) / std[c] (may be NULL); mean3_host / std3_host are HOST pointers to 3 floats. */
int rfx_u8_to_f32_chw(const uint8_t* in, float* raw, float* norm, int N, int H, int W, const float* mean3_host,
                      const float* std3_host, void* stream);

/* Row-pitch change of a (rows, w_src) float32 matrix into (rows, w_dst): copies min(w_src, w_dst) columns per row and
 * zero-fills the rest.  Used to run the correlation on zero-padded copies of maps whose width is not a multiple of 4 (the
 * half-resolution pass of the KITTI driver, evaluation/evalKITTI/evaluation.py:290: 1072/8 = 134 columns) and to crop its
 * output; zero padding on the right is exactly CorrNeigh's own padding (model/model.py:135,143), so results are unchanged. */
int rfx_copy_cols_f32(const float* src, float* dst, long long rows, int w_src, int w_dst, void* stream);

/* ------------------------------------------------------------------------------------------
 * 7x7 local correlation volume (model/model.py:129-160, CorrNeigh.do_forward):
 *     out[n, i*K+j, r, c] = sum_ch x[n,ch,r,c] * y[n,ch,r+i-K/2,c+j-K/2]   (zero outside y)
 * K must be 7 (the only size the reference instantiates: quick_start/align2images.py:38).
 * C must be a multiple of 8.
 * ------------------------------------------------------------------------------------------ */
int rfx_corr_neigh_f32(const float* x, const float* y, float* out, int N, int C, int H, int W, int K,
                       void* stream);
/* Same operation with the tile shape forced (tuning / tests; variant 0 = the automatic choice of rfx_corr_neigh_f32, which
 * returns one of these six): 1 / 2 / 3 = 64 / 32 / 16-row x 16-column tiles; 5 = the tuned 16-row x 80-column kernel (whole
 * 480x640-pair feature-map width: 3 tap groups, hand-pipelined LDS reads, balanced wave map, masked DMA, equal row tiles),
 * 7 / 8 = the tuned kernel with 48- / 64-column tiles.  All six give bit-identical results (channel-ordered fmaf sums).
 * Any other variant -> RFX_E_ARG.  Records inside a group (rfx_group_begin; also rfx_corr_neigh_f32): every problem keeps the
 * tile shape it gets alone, problems of different tile shapes (and the plain kernel of W % 4 != 0) are different kernel
 * instances.  Recording while rfx_corr_timing is enabled -> RFX_E_ARG. */
int rfx_corr_neigh_variant_f32(const float* x, const float* y, float* out, int N, int C, int H, int W, int K,
                               int variant, void* stream);

/* Both directions of a pair in ONE pass over the features -- what PredFlowMask computes with two CorrNeigh calls
 * (evaluation/evalHpatch/evaluation.py:29,34: corr12 = netCorr(featt, featsSample), corr21 = netCorr(featsSample, featt)):
 *     out_xy = CorrNeigh(x, y),   out_yx = CorrNeigh(y, x),   each (N, K*K, H, W).
 * The reverse volume is the forward one at mirrored taps and shifted pixels,
 *     out_yx[n, (K-1-i)*K + (K-1-j), r+i-K/2, c+j-K/2] = out_xy[n, i*K+j, r, c]
 * (the same channel-ordered products, so the values are bit-identical to a second rfx_corr_neigh_f32 call), and zero where
 * the source pixel lies outside the image: the kernel stores every accumulator twice instead of reading 2*C*H*W floats a
 * second time -- (2C + 2K^2)*4 bytes per pixel instead of 2*(2C + K^2)*4.  Requires W % 4 == 0, C % 2 == 0 and 16-byte aligned
 * pointers (the host mirror pads other widths with rfx_copy_cols_f32); K must be 7.  Records inside a group (rfx_group_begin) like
 * rfx_corr_neigh_variant_f32; recording while rfx_corr_timing is enabled -> RFX_E_ARG. */
int rfx_corr_neigh_bidir_f32(const float* x, const float* y, float* out_xy, float* out_yx, int N, int C, int H, int W, int K,
                             void* stream);
/* Kernel-duration capture for the roofline of THIS kernel (bench.py): while a host thread has it enabled, every correlation launch of
 * that thread is issued with hipExtLaunchKernelGGL and a library-owned start / stop event pair attached to the dispatch itself (the
 * timestamps rocprofv3 reads; an event pair recorded around a launch also brackets ~18 us of command-processor work).
 * rfx_corr_timing(enable) returns the previous setting; rfx_corr_timing_collect waits for the captured launches, writes their
 * durations in microseconds in launch order (up to cap; us_out may be NULL), releases the events and returns how many there were. */
int rfx_corr_timing(int enable);
int rfx_corr_timing_collect(float* us_out, int cap);

/* ------------------------------------------------------------------------------------------
 * Warping (kornia HomographyWarper.warp_grid: quick_start/align2images.py:61,65;
 * F.grid_sample: quick_start/align2images.py:66,95,97, evaluation/evalHpatch/evaluation.py:25,45).
 * ------------------------------------------------------------------------------------------ */
/* grid[b,y,x,:] = proj( Hm[b] * (lin(x,w), lin(y,h), 1) ),  lin(i,n) = -1 + 2 i/(n-1).  Records inside a group (rfx_group_begin). */
int rfx_warp_grid_f32(const float* Hm, float* grid, int B, int h, int w, void* stream);

/* bilinear, zeros padding; input (N,C,Hi,Wi), grid (N,Ho,Wo,2) -> out (N,C,Ho,Wo).  Records inside a group (rfx_group_begin). */
int rfx_grid_sample_f32(const float* in, const float* grid, float* out, int N, int C, int Hi, int Wi,
                        int Ho, int Wo, int align_corners, void* stream);

/* Fused fine-flow composition (quick_start/align2images.py:92-95;
 * evaluation/evalHpatch/evaluation.py:40-45,51): up-sample flowDown (N,2,hd,wd) to (H,W) with
 * align_corners=False, add the linspace identity grid, optionally clamp to [-1,1], sample the coarse
 * grid (N,Hc,Wc,2) there (bilinear, zeros, align_corners=False) -> flow12 (N,H,W,2).  (Hc,Wc) = (H,W) everywhere except in
 * the full-resolution pass of the KITTI driver, which composes at the ORIGINAL image size on a coarse grid of the
 * fine-stage size (evaluation/evalKITTI/evaluation.py:302 with :49-81).  If inb != NULL it
 * receives the in-bounds mask (N,H,W) = (-1<=fx<=1)&(-1<=fy<=1) as 0/1 floats; if flowUp != NULL it
 * receives the (clamped) sampling grid (N,H,W,2).  Records inside a group (rfx_group_begin). */
int rfx_compose_flow_f32(const float* flowDown, const float* coarseGrid, float* flow12, float* inb,
                         float* flowUp, int N, int hd, int wd, int Hc, int Wc, int H, int W, int clamp, void* stream);

/* The tail of model.predFlowCoarse / predFlowCoarseNoGrad (model/model.py:333-340, 344-350): flowCoarse (B,2,H,W) is the
 * NetFlowCoarse output; flow (B,H,W,2) = clamp(flowCoarse.permute(0,2,3,1) + grid, -1, 1) with grid (grid_batch,H,W,2),
 * grid_batch = 1 (broadcast) or B; flowGrad (B,1,H-1,W-1) = L2 norm over the two channels of
 * flowCoarse[:, :, 1:, 1:] - flowCoarse[:, :, :-1, :-1], or NULL (the NoGrad variant). */
int rfx_flow_grad_clamp_f32(const float* flowCoarse, const float* grid, float* flowGrad, float* flow, int B, int H, int W,
                            int grid_batch, void* stream);

/* Multi-homography merge of the offline flow assembly (evaluation/evalHpatch/getResults.py:48-61,
 * evaluation/evalCorr/getResults.py:121-134, evaluation/evalKITTI/getResults.py:126-138).
 * flow (n,HW,2) composed flows; match12 = up-sampled matchability of homography i at match12 + i*match12_stride;
 * cyc (n,HW) = grid_sample(up(match21), flowUp) or NULL; inb (n,HW) in-bounds mask or NULL.
 * score_i = match12_i * cyc_i * inb_i (left to right).  Pixel owner: homography 0 if score_0 >= th, otherwise the
 * first i >= 1 with score_i >= th (only when multiH != 0), otherwise 0.  Outputs: flowGlobal (HW,2) = owner's flow
 * clamped to [-1,1]; matchGlobal (HW) = owner's score (may be NULL); binary (HW) u8 = "some score reached th"
 * (may be NULL). */
int rfx_merge_multi_h_f32(const float* flow, const float* match12, long long match12_stride, const float* cyc,
                          const float* inb, int n, long long HW, float th, int multiH, float* flowGlobal,
                          float* matchGlobal, uint8_t* binary, void* stream);

/* score (n,HW) = match12_i * cyc_i * inb_i (same operands and order as above; cyc / inb may be NULL): the "match"
 * tensor of evaluation/evalKITTI/getResults.py:120, materialised when a host-side filter (remove_small_cc, :122)
 * runs before the merge -- rfx_merge_multi_h_f32 is then called with cyc = inb = NULL on the filtered scores. */
int rfx_match_score_f32(const float* match12, long long match12_stride, const float* cyc, const float* inb, int n,
                        long long HW, float* score, void* stream);

/* The tail of the cycle-checked PredFlowMask forms (evaluation/evalYFCC/evaluation.py:47-58, evaluation/evalKITTI/evaluation.py:66-81)
 * as one kernel: per pixel what rfx_resize_bilinear_f32 (align_corners = 0) of both matchability maps, rfx_compose_flow_f32 with
 * clamp = 1, inb and flowUp, rfx_grid_sample_f32 of the up-sampled match21 at flowUp and rfx_match_score_f32 compute, operation for
 * operation and bit for bit, without the up-sampled maps, flowUp, inb and the sampled cycle map in memory.
 * flowDown8 (N,2,hd,wd); match12Down8 / match21Down8: N planes of hd*wd floats, image i at + i*stride (the two halves of one
 * (2N,1,hd,wd) tensor: stride hd*wd); coarseGrid (N,Hc,Wc,2); outputs at (H,W) -- (Hc,Wc) everywhere except in the KITTI
 * full-resolution pass (evaluation/evalKITTI/evaluation.py:302) -- flow12 (N,H,W,2) and match (N,H,W) = (match12 * cycle) * inb,
 * both caller-owned (views of packed buffers); no input may alias an output.  Records inside a group (rfx_group_begin). */
int rfx_cycle_tail_f32(const float* flowDown8, const float* match12Down8, long long match12_stride, const float* match21Down8,
                       long long match21_stride, const float* coarseGrid, float* flow12, float* match, int N, int hd, int wd,
                       int Hc, int Wc, int H, int W, void* stream);

/* The offline flow assembly of the HPatches, Corr and YFCC scripts (evaluation/evalHpatch/getResults.py:16-63,
 * evaluation/evalCorr/getResults.py:78-136, evaluation/evalYFCC/getResults.py:150-190) for EVERY pair of a batch, straight from the
 * result records of the multi-homography drivers, in ONE launch (ADDED under ABI 17: nothing existing moves).  Per pair b with
 * n = nbH read from its record ON THE DEVICE (clamped to max_h; only homography 0 when multiH == 0) the outputs are, bit for bit,
 * those of rfx_warp_grid_f32(H[:n]) -> rfx_compose_flow_f32(flowDown8[:n], clamp = 1, inb[, flowUp]) -> rfx_resize_bilinear_f32(
 * matchDown8[:n], align_corners = 0) [-> cycle != 0: rfx_grid_sample_f32(up-sampled match21, flowUp)] -> rfx_merge_multi_h_f32(th,
 * multiH) -- without any (n,H,W) intermediate: a thread walks the homographies of its pixel in the merge's order, stops at the owner,
 * and forms a tap of a homography's coarse grid (H x W, the output size) from the nine numbers.  A pair with nbH == 0 gets zeros.
 * rec: rec_elems floats, rows of `width` floats laid out as rfx_multih_accept_f32 / rfx_multih_accept_ragged_f32 fill them: [0] nbH,
 * H (max_h,9) from off_H, flowDown8 (max_h,2,h8,w8) from off_flow, matchDown8 (max_h,2,h8,w8) (channel 0: 1->2, channel 1: 2->1)
 * from the pair's off_match.  table (B,8) int64 on the device, row b: element offset of the pair's row in rec | h8 | w8 | off_match |
 * H | W (output size) | pixel offset of the pair's maps in the packed outputs | 0 -- a pure function of the batch's size lists.
 * A row that does not describe a record inside rec and a map inside the outputs is skipped.  max_hw = the largest H * W (sizes the
 * grid; 8192 workgroups per pair at the most, larger maps take several trips).  bg: total_px bytes laid out like binary, or NULL;
 * binary &= bg != 0 (YFCC), nothing else changes.  Outputs, total_px pixels each: flowGlobal (total_px,2) 8-byte aligned = the
 * owner's flow clamped to [-1,1] with NaN kept, matchGlobal = the owner's score (score_0 where nobody reaches th), binary u8.
 * No output may alias rec.  KITTI's two-level composition and component filter are not covered. */
int rfx_assemble_records_f32(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                             const long long* table, int B, long long max_hw, float th, int multiH, int cycle,
                             const uint8_t* bg, float* flowGlobal, float* matchGlobal, uint8_t* binary, long long total_px,
                             void* stream);

/* The KITTI form of the assembly above (evaluation/evalKITTI/getResults.py:95-141, getFlow_all) for EVERY pair of a batch, from the
 * records of the KITTI drivers, which carry the half-resolution flowD2 (both ADDED under ABI 17: nothing existing moves).  Per pair
 * with n = nbH read on the device the outputs are, bit for bit, those of rfx_warp_grid_f32(H[:n]) -> rfx_compose_flow_f32(flowD2[:n],
 * clamp = 1) -> rfx_compose_flow_f32(flowDown8[:n], that grid, clamp = 1, inb, flowUp) -> rfx_resize_bilinear_f32(matchDown8[:n]) ->
 * rfx_grid_sample_f32(up-sampled match21, flowUp) -> [rfx_match_score_f32 -> rfx_remove_small_cc_f32 ->] rfx_merge_multi_h_f32:
 * a tap of the fine flow's sample is the d2 flow at the tap's integer pixel, itself a four-tap sample of the homography grid formed
 * from the nine numbers; neither d2, flowUp, inb nor an up-sampled map is stored.
 * rec, width, max_h, off_H, off_flow: as for rfx_assemble_records_f32; a row also holds flowD2 (max_h,2,hd2,wd2) from the pair's
 * off_d2.  table (B,12) int64 on the device, row b:
 *     [0] element offset of the pair's row in rec | [1] h8 | [2] w8 | [3] off_match | [4] off_d2 | [5] hd2 | [6] wd2 | [7] H | [8] W
 *     (output size) | [9] pixel offset of the pair's maps in the packed outputs | [10] element offset of the pair's score map 0 in
 *     the batch's packed scores (map i at + i * H * W, max_h maps per pair) | [11] max_area of the component filter for H * W
 * -- a pure function of the batch's size lists and cc_th.  A row that does not describe a record inside rec, a map inside the outputs
 * and (where scores are used) max_h maps inside the score buffer is skipped.  max_hw = the largest H * W (8192 workgroups per pair at
 * the most, larger maps take further trips).  The score buffer `scores` holds the elements [score_base, score_base + score_elems) of
 * the batch's packed scores: a call on a chunk of consecutive pairs passes the chunk's first table row, its B and its own base.
 * Limits (RFX_E_LIMIT): max_hw, total_px, score_elems <= 2^31 - 1, B * max_h <= 65535.  Both take a stream, allocate nothing and do
 * not sync.
 *
 * rfx_kitti_scores_records_f32 (only with a component filter, cc_th > 0): score_i = (up(match12_i) * sample(up(match21_i), flowUp_i))
 * * inb_i -- rfx_match_score_f32's map -- for every i < last of every pair (last = nbH with multiH, else min(nbH, 1)) into scores,
 * and row b * max_h + i of dims (B * max_h, 3) int32, the table rfx_remove_small_cc_ragged_f32 reads: (H, W, max_area) for i < last,
 * (0, 0, 0) -- a map the filter skips -- otherwise.  The filter's match_off is the host's: table[b][10] - score_base + i * H * W.
 *
 * rfx_assemble_kitti_records_f32: scores == NULL (cc_th == 0): a thread walks the homographies of its pixel in the merge's order and
 * stops at the owner -- ONE launch for the batch.  scores != NULL: the thread finds the owner on the FILTERED scores by the same
 * rule and evaluates the owner's flow only; matchGlobal is the owner's filtered score, or filtered score_0 where nobody reaches th.
 * Outputs as rfx_assemble_records_f32 (flowGlobal 8-byte aligned, NaN kept by the clamp); a pair with nbH == 0 gets zeros.  No
 * output may alias rec or scores. */
int rfx_kitti_scores_records_f32(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                                 const long long* table, int B, long long max_hw, int multiH, float* scores, long long score_base,
                                 long long score_elems, int32_t* dims, long long total_px, void* stream);
int rfx_assemble_kitti_records_f32(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                                   const long long* table, int B, long long max_hw, float th, int multiH, const float* scores,
                                   long long score_base, long long score_elems, float* flowGlobal, float* matchGlobal,
                                   uint8_t* binary, long long total_px, void* stream);

/* The small-component filter of the KITTI scripts (evaluation/evalKITTI/evaluation.py:85-100 online -- remove_small_cc(match,
 * 0.99, cc_th) at :321 -- and evaluation/evalKITTI/getResults.py:66-84 offline, :122), which the reference runs on the host
 * with skimage.measure.label: out = in with every 8-connected component of (in > match_th) of at most max_area pixels set to
 * zero, per image of the (N,H,W) batch.  max_area = the largest pixel count a with a / (H*W) <= cc_th in float64 (the host
 * mirrors compute it so; the reference's test is on the area FRACTION).  ws: rfx_remove_small_cc_ws_bytes(N,H,W) bytes.
 * Exact: the result of a labelling does not depend on the label numbering.  in and out may be the same buffer. */
size_t rfx_remove_small_cc_ws_bytes(int N, int H, int W);
int rfx_remove_small_cc_f32(const float* in, float* out, int N, int H, int W, float match_th, int max_area, void* ws,
                            void* stream);

/* (ABI 14) The same filter for n_active maps of DIFFERENT sizes in one launch chain (a round of the KITTI driver on a ragged batch):
 * map k is h_k * w_k floats at element offset match_off[k] (n_active int64) of ONE packed buffer of total_px floats -- the layout
 * rfx_multih_accept_ragged_f32 consumes, so the filter runs in place between the fine stage and the accept kernel -- and row k of the
 * device table dims (n_active,3) int32 holds h_k, w_k and the map's OWN max_area_k (the bound above formed with h_k * w_k).  Maps
 * must not overlap; a table row that does not lie inside the buffer is skipped.  Every map is labelled on its own (segments, rows
 * and unions are relative to the map's origin; "a component that is the whole image stays" uses h_k * w_k), so map k's output is,
 * bit for bit, rfx_remove_small_cc_f32 on that map alone.  max_hw = the largest h_k * w_k (sizes the grid).  Limits: total_px <=
 * 2^31 - 1, n_active <= 65535 (RFX_E_LIMIT).  ws: rfx_remove_small_cc_ragged_ws_bytes(total_px) = three int32 per packed pixel.
 * in and out may be the same buffer; pixels of the buffer that belong to no map are neither read nor written. */
size_t rfx_remove_small_cc_ragged_ws_bytes(long long total_px);
int rfx_remove_small_cc_ragged_f32(const float* in, float* out, const long long* match_off, const int32_t* dims, int n_active,
                                   long long total_px, long long max_hw, float match_th, void* ws, void* stream);

/* The nearest-explained-pixel fill of the KITTI scripts' --interpolate option (evaluation/evalKITTI/getResults.py:87-93,
 * interpolate_flow_match: scipy.ndimage.distance_transform_edt(~binary, return_indices=True) on the host there, then flow[idx]).
 * values, out (N,H,W,C) float32, channels last -- the layout of flowGlobal; explained (N,H,W) bytes (a torch.bool), non-zero = the
 * pixel keeps its value.  out[n,r,x,:] = values[n,r',c',:] with (r',c') scipy's index for pixel (r,x), INDEX FOR INDEX: the
 * explained pixel of map n that minimises (r'-r)^2 + (c'-x)^2 (an exact integer), among equals the smallest column c', among those
 * the smallest row r'.  A map without any explained pixel: scipy's index is (-1, 0) everywhere, which numpy's indexing reads as
 * pixel (H-1, 0); out takes that pixel's values.  index, if not NULL, receives the index pairs (N,2,H,W) int32 -- scipy's layout
 * per map, row plane first; (-1, 0) for such an empty map.  Values move as 32-bit words: NaN payloads and -0.0 arrive bit for bit.
 * Two launches (a sweep per column, then a search per row over the columns' nearest rows, staged in 32 KB of LDS).
 * ws: rfx_nearest_fill_ws_bytes(N,H,W) bytes = one int32 per pixel (0 for a non-positive size).
 * RFX_E_ARG: a null pointer other than index, a non-positive N, H, W or C, out == values (the kernel reads other pixels while it
 * writes).  RFX_E_LIMIT: W > 8192 (the staged row), H > 31728 (distances stay int32 below the no-pixel sentinel 2^30), C > 8.
 * All of these are checked before any HIP call. */
size_t rfx_nearest_fill_ws_bytes(int N, int H, int W);
int rfx_nearest_fill_f32(const float* values, const unsigned char* explained, float* out, int32_t* index, int N, int H, int W, int C,
                         void* ws, void* stream);

/* The pixel correspondences of all explained pixels of an assembled flow (evaluation/evalYFCC/getResults.py:53-71,
 * matches_from_flow: numpy boolean indexing of the flow and of np.rot90(gridB, k) on the host there).
 * flow (N,H,W,2) float32, keep (N,H,W) bytes, non-zero = explained; bg (N,H,W) bytes or NULL, ANDed with keep (the script's
 * match_binary * matchBG).  k in 0..3 = (angle / 90) mod 4; (wA, hA) the source size, (wB, hB) the UNROTATED target size: the maps
 * are (hB, wB) for even k and (wB, hB) for odd k.  Rows come map after map, row-major over the pixels (i, j) of a map:
 *     pts1 (rows,2) float32:  t = x + 1; t = t * (float)(wA - 1); t = t / 2, each step rounded to float32; y with hA - 1;
 *     pts2 (rows,2) int64:    np.rot90(gridB, k)[i, j] = (j, i) | (wB-1-i, j) | (wB-1-j, hB-1-i) | (i, hB-1-j) for k = 0 | 1 | 2 | 3;
 *     offsets (N+1) int64:    the exclusive prefix of the per-map row counts, offsets[N] = rows; stays on the device.
 * pts1 and pts2 must have room for N*H*W rows; rows beyond offsets[N] are not written.  Deterministic: three stream-ordered launches
 * (count per 1024-pixel tile, one-workgroup scan of the tile counts, scatter by recomputed ballots), no atomics, no workgroup waits
 * on another; flow is read only where kept.  ws: rfx_flow_points_ws_bytes(N,H,W) bytes = one int32 per tile, ceil(H*W / 1024) tiles
 * per map (0 for a non-positive size).
 * RFX_E_ARG: a null pointer other than bg, a non-positive N, H or W, k outside 0..3, wA or hA < 1, a map shape that is not the
 * one k and (wB, hB) give, flow / pts1 / offsets not 8-byte or pts2 not 16-byte aligned.  RFX_E_LIMIT: N*H*W > 2^31 - 1.
 * All of these are checked before any HIP call. */
size_t rfx_flow_points_ws_bytes(int N, int H, int W);
int rfx_flow_points_f32(const float* flow, const unsigned char* keep, const unsigned char* bg, int N, int H, int W, int k, int wA,
                        int hA, int wB, int hB, float* pts1, long long* pts2, long long* offsets, void* ws, void* stream);

/* rfx_flow_points_f32 for B maps of DIFFERENT sizes, each with its own quarter turn and its own source size, in one chain (ADDED
 * under ABI 17, like rfx_keep_mask_ragged_f32: nothing existing moves): evaluation/evalYFCC/getResults.py:53-71 (matches_from_flow)
 * as the script's loop :298-318 calls it once per pair, for a whole batch.
 * flow (total_px,2) float32, keep (total_px) bytes, bg (total_px) bytes or NULL: the packed buffers rfx_assemble_records_f32 fills
 * for a ragged batch -- map b's pixels at its pixel offset, row-major.  table (B,8) int64 on the device, row b:
 *     pixel offset | H | W | k | wA | hA | index of the map's first tile | 0
 * a pure function of the size lists: a map of H*W pixels has ceil(H*W / 1024) tiles, the first-tile column is their exclusive
 * prefix, total_tiles their sum.  (wB, hB) follow from (H, W, k): the map is (hB, wB) for even k and (wB, hB) for odd k.
 * The rule is rfx_flow_points_f32's, applied per map with that map's k, wA, hA, wB, hB; rows come map after map, row-major inside a
 * map; offsets (B+1) int64 = the rows before each map, offsets[B] = all rows, stays on the device; a map without a kept pixel
 * contributes no row.  pts1 and pts2 must have room for total_px rows; rows beyond offsets[B] are not written, and no row at or
 * beyond total_px is ever written, whatever ws holds.  Deterministic: three stream-ordered launches (count per tile, the map of a
 * tile found by a binary search over the first-tile column; one-workgroup scan; scatter by recomputed ballots), no atomics, no
 * workgroup waits on another; both tiled grids are capped at 8192 workgroups and stride.
 * ws: rfx_flow_points_ragged_ws_bytes(total_tiles) bytes = one int32 per tile (0 for a non-positive count).
 * A table row that does not describe a map inside the buffers (a negative offset, a non-positive size, offset + H*W > total_px, k
 * outside 0..3, wA or hA outside 1..2^31-1, a first tile that is negative or behind the tile looked up) is skipped: none of its
 * pixels is read, it contributes no row.
 * RFX_E_ARG: a null pointer other than bg, a non-positive B, total_px or total_tiles, total_tiles > total_px, flow / table / pts1 /
 * offsets not 8-byte or pts2 not 16-byte aligned.  RFX_E_LIMIT: total_px > 2^31 - 1, B > 65535.  All of these are checked before
 * any HIP call. */
size_t rfx_flow_points_ragged_ws_bytes(long long total_tiles);
int rfx_flow_points_ragged_f32(const float* flow, const unsigned char* keep, const unsigned char* bg, const long long* table, int B,
                               long long total_px, long long total_tiles, float* pts1, long long* pts2, long long* offsets, void* ws,
                               void* stream);

/* The keypoint transfer of evaluation/evalCorr/getResults.py:15-31 (alignmentError: the whole maps go to the host there): for K
 * target pixels (xb[q], yb[q]) (int32, device) of ONE map, flow (H,W,2), match (H,W) float32,
 *     xa[q] = ((flow[yb,xb,0] + 1) * 0.5f) * (float)(wA - 1),  ya[q] with channel 1 and hA - 1 (float32, in that order),
 *     keep[q] = match[yb,xb] > 0.5f  (a byte).
 * A pixel outside the map reads nothing and gives 0, 0, 0 (the Python mirror refuses it on the host).
 * RFX_E_ARG: a null pointer, a non-positive K, H or W, wA or hA < 1, flow not 8-byte aligned; RFX_E_LIMIT: H*W > 2^31 - 1. */
int rfx_sample_points_f32(const float* flow, const float* match, const int32_t* xb, const int32_t* yb, int K, int H, int W, int wA,
                          int hA, float* xa, float* ya, unsigned char* keep, void* stream);

/* The sparse-correspondence results step of a whole batch from the drivers' records, without the dense maps (both ADDED under ABI 17,
 * like rfx_keep_mask_ragged_f32: nothing existing moves).
 *
 * rfx_records_keypoints_f32: evaluation/evalCorr/getResults.py:78-136 (getFlow) read at the annotated pixels as :15-31
 * (alignmentError) and :281-282 (the threshold loop) read it.  rec, rec_elems, width, max_h, off_H, off_flow, table (B,8), th, multiH,
 * cycle, bg: as rfx_assemble_records_f32 takes them, with the same row checks; total_px = the pixels of all pairs' maps in that
 * layout (what bg holds; a row's map must lie inside it).  ktable (B,4) int64 on the device, row b:
 *     first keypoint | number of keypoints | wA | hA
 * the first-keypoint column the exclusive prefix of the counts; xb, yb (K_total) int32: the target pixels, pair after pair.  One
 * thread per keypoint finds its pair by a binary search over the first-keypoint column and evaluates the pixel from the record alone:
 *     xa[q] = ((flowGlobal[yb,xb,0] + 1) * 0.5f) * (float)(wA - 1), ya[q] with channel 1 and hA - 1 (float32, in that order);
 *     m[q] = matchGlobal[yb,xb];  flag[q] bit 0 = binary[yb,xb] (ANDed with bg when given), bit 1 = both flow channels in [-1, 1]
 *     (the flow is clamped: clear only for a NaN).
 * Per pair bit for bit what rfx_assemble_records_f32 followed by rfx_sample_points_f32 gives at the same pixels.  A keypoint outside
 * its map, or of a row that is refused, reads nothing and gives 0, 0, 0, 0; a pair with nbH < 1 gives what its zero maps give.  No
 * atomics, no LDS.
 * RFX_E_ARG: a null pointer other than bg, a non-positive B, width, max_h, total_px or K_total, offsets that do not describe a
 * record, rec_elems < B * width, a table not 8-byte aligned.  RFX_E_LIMIT: B > 65535, total_px or K_total > 2^31 - 1.
 *
 * rfx_pck_tally_f64: evaluation/evalCorr/getResults.py:281-282 (which keypoints a matchability threshold keeps), :25-36 (distances
 * and their tally under the pixel grid) and :273-277 (a pair without a flow).  xa, ya, m, flag: the outputs above; xs, ys (K_total)
 * int32 the source keypoints; ktable as above; match_th (M) float32; grid (T) float64, T <= 16; valid (B) bytes or NULL.
 * For threshold t: keep = (m >= t) && flag bit 1 when t > 0, every keypoint (a NaN included) when t <= 0;
 *     d = sqrt((double(xa) - xs)^2 + (double(ya) - ys)^2), every float64 step rounded on its own (no fused multiply-add);
 *     counts[t,b,j] = kept keypoints of pair b with d <= grid[j] (int64, (M,B,T));  nb[t,b] = kept keypoints (int64, (M,B));
 *     dist (M,K_total) float64 or NULL: d, NaN where the keypoint is not kept.
 * A pair with valid[b] == 0: nb = its number of keypoints, counts zero, dist NaN.  One workgroup per (threshold, pair): ballots and
 * popcounts per wavefront, one LDS pass, thread 0 writes; no atomics; integer sums, the same bits every run.  K_total may be 0.
 * RFX_E_ARG: a null ktable, match_th, grid, counts or nb, a null keypoint array with K_total > 0, a non-positive B, M or T, T > 16,
 * K_total < 0, ktable / grid / counts / nb / dist not 8-byte aligned.  RFX_E_LIMIT: B > 65535, K_total > 2^31 - 1. */
int rfx_records_keypoints_f32(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                              const long long* table, int B, long long total_px, float th, int multiH, int cycle, const uint8_t* bg,
                              const long long* ktable, const int32_t* xb, const int32_t* yb, long long K_total, float* xa, float* ya,
                              float* m, uint8_t* flag, void* stream);
int rfx_pck_tally_f64(const float* xa, const float* ya, const float* m, const uint8_t* flag, const int32_t* xs, const int32_t* ys,
                      const long long* ktable, int B, long long K_total, const float* match_th, int M, const double* grid, int T,
                      const uint8_t* valid, long long* counts, long long* nb, double* dist, void* stream);

/* The end-point error of an assembled flow, reduced on the device to one float64 sum and one count per map (ADDED under ABI 17, like
 * rfx_keep_mask_ragged_f32: nothing existing moves).  Both entry points below share the outputs and the reduction:
 *     sum (N) float64:    the counted pixels' errors added in float64, in an order fixed by the pixel's place in its map;
 *     count (N) int32:    the number of counted pixels;
 *     err (N,H,W) or NULL: the per-pixel error, NaN (the quiet NaN 0x7fc00000 / 0x7ff8000000000000) where the pixel is not counted.
 * Two stream-ordered launches, no floating-point atomics, no workgroup waits on another: a workgroup adds a tile of 1024 consecutive
 * pixels of ONE map (a thread its four pixels in order, a wavefront by a fixed tree, the four wavefronts in order) and writes the
 * tile's sum and count to ws; one wavefront per map then adds the map's tile sums in index order.  A pixel that is not counted adds
 * +0.0.  A map's sum therefore has the same bits run after run, alone or at any position of a batch; a single counted pixel gives its
 * own error exactly.  ws: rfx_epe_ws_bytes(N,H,W) bytes = one float64 and one int32 per tile, ceil(H*W / 1024) tiles per map (0 for a
 * non-positive size).
 *
 * rfx_epe_homography_f32: evaluation/evalHpatch/getResults.py:83-144 (getGT), :147-156 (epe) and the statements :221-250 that mask
 * and un-normalise the two maps.  flow (N,Sh,Sw,2) float32, Hinv (N,9) float64 row-major (the inverse of the scaled ground-truth
 * homography).  Per pixel (i, j): (xw, yw, zw) = Hinv (j, i, 1) in float64, each row as (h0 * j + h1 * i) + h2 without a fused step,
 * rounded to float32; gx = ((2 * xw) / (zw + 1e-8f)) / (float)(Sw - 1) - 1 in float32 steps, gy with yw and Sh - 1; counted iff
 * -1 <= gx <= 1 and -1 <= gy <= 1; both maps to pixels by t = v + 1, t = t * (float)(S - 1), t = t / 2 (Sw for x, Sh for y);
 * err = sqrtf(fmaf(dy, dy, dx * dx)) -- what torch.norm(p=2, dim=1) gives a two-element row on the CPU.  err is float32.
 *
 * rfx_epe_flow_f32: evaluation/evalKITTI/getResults.py:221-228.  flow (N,H,W,2) float32 (absolute, in [-1,1]), u, v (N,H,W) float32
 * (KITTI's (uint16 - 32768) / 64 is exact in float32), valid (N,H,W) bytes, non-zero = counted.
 * up = ((fx - linspace(-1,1,W)[j]) * (float)(W - 1)) / 2 in float32 steps, vp with H; err = sqrt(dx * dx + dy * dy) in float64 with
 * dx = (double)up - (double)u.  err is float64.
 *
 * RFX_E_ARG: a null pointer other than err, a non-positive N, H or W, Sh or Sw < 2, flow / Hinv / sum / ws / a float64 err not
 * 8-byte aligned.  RFX_E_LIMIT: N*H*W > 2^31 - 1.  All of these are checked before any HIP call. */
size_t rfx_epe_ws_bytes(int N, int H, int W);
int rfx_epe_homography_f32(const float* flow, const double* Hinv, int N, int Sh, int Sw, double* sum, int32_t* count, float* err,
                           void* ws, void* stream);
int rfx_epe_flow_f32(const float* flow, const float* u, const float* v, const unsigned char* valid, int N, int H, int W, double* sum,
                     int32_t* count, double* err, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * All-pairs correlation + mutual nearest neighbours (utils/outil.py:32-45, mutualMatching).
 * featA: (C, nA) and featB: (C, nB), column = one cell ("K-major": element (k,i) at k*ld+i).
 * maskB (optional, nB floats, 0/1) multiplies featB's columns (quick_start/coarseAlignFeatMatch.py:143).
 * Outputs: idx1/idx2 (int64, capacity min(nA,nB)) in ascending idx1 order, count (int32[1]).
 * The nA x nB score matrix is never written to memory.  A score -- a sum of C non-negative products -- is accumulated in chunks of
 * 256 products (default; argument score_chunk) that are added to a running total (round 4): the chain's round-off over C = 1024 is
 * 2.8x that of the reference's torch.mm and flipped float64 near-ties of the arg-max 1.5-2.3x as often as the reference flips them
 * against itself; chunked: 1.0-1.1x on the 64 bench pairs, 1.25x over 128 / 160 pairs.
 * ws: rfx_mutual_nn_ws_bytes(nA, nB) bytes.
 * ------------------------------------------------------------------------------------------ */
size_t rfx_mutual_nn_ws_bytes(int nA, int nB);
/* (ABI 8) score_chunk: how a score's C products are summed -- an fma chain inside chunks of `score_chunk` consecutive products
 * (a multiple of 32), the chunk sums added to a running total in k order.  0 = the library default, 256 products; < 0 = ONE chain
 * over all C.  The reference's score is torch.mm on the HOST (utils/outil.py:34): MKL's sgemm sums k as an fma chain inside blocks
 * of KC products and adds the block sums to C -- KC = 192 on the GPU box's EPYC host, 384 on a Xeon (scripts/mm_blocking_probe.py).
 * With score_chunk = KC the device's scores equal that host's torch.mm BIT FOR BIT on equal features, so that what is left of the
 * arg-max near-tie flips comes from the trunk features alone.  It is an ARGUMENT of every call (ABI 7 had a process-wide setter):
 * two pipelines of one process, or two ranks, never share it by accident; the Python mirror resolves it ONCE per pipeline
 * (rfx/ops.py::resolve_score_chunk: an explicit value, or a probe of the host's KC) and records it in its results.
 * Returns RFX_E_ARG for a positive score_chunk that is not a multiple of 32. */
int rfx_mutual_nn_f32(const float* featA, int ldA, int nA, const float* featB, int ldB, int nB, int C,
                      const float* maskB, int64_t* idx1, int64_t* idx2, int32_t* count, void* ws, int score_chunk,
                      void* stream);

/* The same for `batch` independent pairs in one launch (blockIdx.y = pair): pair b reads featA + b*strideA,
 * featB + b*strideB, maskB + b*nB, writes idx1/idx2 + b*min(nA,nB), count[b], and uses ws + b*ws_bytes(nA,nB). */
int rfx_mutual_nn_batched_f32(const float* featA, int ldA, int nA, long long strideA, const float* featB, int ldB,
                              int nB, long long strideB, int C, const float* maskB, int64_t* idx1, int64_t* idx2,
                              int32_t* count, void* ws, int batch, int score_chunk, void* stream);

/* (ABI 11) Ragged batch: `batch` pairs of DIFFERENT sizes in one tile -> reduce -> compact launch chain (utils/outil.py:32-45 and the
 * mask multiply of quick_start/coarseAlignFeatMatch.py:143, per pair).  nA, nB: (batch) int32 DEVICE arrays, pair b's own sizes,
 * at most maxNA <= ldA / maxNB <= ldB (the host's maxima: they size the grid).  Features on a common padded layout: pair b reads
 * the first nA[b] columns of featA + b*C*ldA (C,ldA) and the first nB[b] of featB + b*C*ldB (C,ldB); maskB (batch,ldB) or NULL.
 * Pair b writes idx1/idx2 + b*cap ((batch,cap) int64, cap >= min(nA[b], nB[b])) and count[b], and uses the workspace slot
 * ws + b*rfx_mutual_nn_ws_bytes(maxNA, maxNB).  Tiles past a pair's own grid exit at once; a pair with sizes out of range gets
 * count 0.  Same k order, score_chunk chunking and tie rule as rfx_mutual_nn_f32: a pair's indices and count equal, bit for
 * bit, a single-pair call on its own features.  Requires C % 32 == 0 and C >= 64. */
int rfx_mutual_nn_ragged_f32(const float* featA, int ldA, const float* featB, int ldB, const int32_t* nA, const int32_t* nB,
                             int maxNA, int maxNB, int C, const float* maskB, int64_t* idx1, int64_t* idx2, int cap,
                             int32_t* count, void* ws, int batch, int score_chunk, void* stream);

/* ------------------------------------------------------------------------------------------
 * RANSAC over 4-point DLT homographies (utils/outil.py:68-164).
 * match1/match2: (n,3) source / target points (x,y,1); samples: (N,4) int64 indices into them.
 * ------------------------------------------------------------------------------------------ */
/* outil.Homography (utils/outil.py:68-87): per hypothesis the unit-norm null vector of the 8x9 DLT
 * system in float64 with LAPACK dgesdd's sign (dgebd2 Householder sweep), cast to float32.
 * X,Y: (N,4,3) source / target samples -> Hout (N,3,3). */
int rfx_dlt4_homography(const float* X, const float* Y, int N, float* Hout, void* stream);

/* outil.Prediction (utils/outil.py:97-100): reprojection error ||X[:, :2] - proj(Y H^T)||_2 for every
 * (hypothesis, match) pair, float32 in the reference's operation order.  match1/match2 (n,3), Hs (N,3,3)
 * -> err (N,n).  N <= 65535. */
int rfx_prediction_f32(const float* match1, const float* match2, int n, const float* Hs, int N, float* err,
                       void* stream);

/* outil.ScoreRANSAC (utils/outil.py:102-113): H per hypothesis + inlier count * (det(H) > 1e-6).
 * Hout (N,3,3) f32, counts (N) int64.  ws: rfx_ransac_ws_bytes(n, N).
 * flags_out (ABI 8; optional, N bytes): the per-hypothesis flags of the SAME DLT pass -- bit 0 evaluated, bit 1 det gate passed,
 * bit 2 the 8x9 system is rank deficient (dlt.h: one Sturm count on the bidiagonal) -- for a caller that re-solves exactly those
 * hypotheses with the host's LAPACK (rfx/ops.py::score_hypotheses(degenerate="lapack")); NULL skips the rank test. */
int rfx_score_hypotheses(const float* match1, const float* match2, int n, const int64_t* samples, int N,
                         float tol, float* Hout, int64_t* counts, uint8_t* flags_out, void* ws, void* stream);

/* outil.RANSAC (utils/outil.py:117-164) given the index draw: duplicate filter (:122-133), chunks of
 * 100 with the zero-chunk abort (:140-146), tail chunk (:153-160), first-maximum selection, final
 * inlier mask (:162-163).
 * result (int32[4]): [0] status 0 = ok, 1 = aborted (reference returns (None,0,[],[])), 2 = no
 * hypothesis beat 0 (reference raises TypeError); [1] best inlier count; [2] index of the winning
 * hypothesis in `samples`; [3] number of hypotheses that survived the duplicate filter.
 * bestH (9 f32), inlier (n uint8).  ws: rfx_ransac_ws_bytes(n, N). */
size_t rfx_ransac_ws_bytes(int n, int N);
int rfx_ransac_h4(const float* match1, const float* match2, int n, const int64_t* samples, int N,
                  float tol, float* bestH, uint8_t* inlier, int32_t* result, void* ws, void* stream);

/* The same for a whole batch of pairs in ONE launch chain (pack, DLT, count, select with blockIdx.y = pair): what the
 * per-pair host loop around outil.RANSAC (quick_start/coarseAlignFeatMatch.py:157-170, once per pair) costs in launches
 * and host round trips.  match1/match2 (batch,cap,3); n (batch) int32 ON THE DEVICE = matches of each pair (<= cap);
 * samples (batch,N,4) int64; bestH (batch,9); inlier (batch,cap) uint8; result (batch,4) as above with the extra
 * status 3 = fewer than nbPoint (4) matches (the reference returns its None sentinel before calling RANSAC,
 * quick_start/coarseAlignFeatMatch.py:157-158).  Per pair bit-identical to rfx_ransac_h4.  batch <= 65535.
 * ws: rfx_ransac_batched_ws_bytes(cap, N, batch). */
size_t rfx_ransac_batched_ws_bytes(int cap, int N, int batch);
int rfx_ransac_h4_batched(const float* match1, const float* match2, const int32_t* n, int cap, const int64_t* samples,
                          int N, float tol, float* bestH, uint8_t* inlier, int32_t* result, void* ws, int batch,
                          void* stream);

/* Rank-deficient 4-point samples (utils/outil.py:84: ``np.linalg.svd(A)`` on an 8x9 system of rank 7).  Three matched points
 * collinear in BOTH images -- common on the feature-cell lattices -- leave a two-dimensional null space; which unit vector of
 * it LAPACK's Vh[8] is depends on rounding inside the host BLAS (it differs between LAPACK builds), so no device restatement
 * can be bit-exact there.  The DLT kernel therefore FLAGS such hypotheses (sigma_8 < 1e-8 * max|bidiagonal|, one Sturm count on
 * the bidiagonal dgebd2 leaves; csrc/dlt.h) and the search can be run in two stages around a host re-solve:
 *   rfx_ransac_h4_batched_stage(..., stages = 1)   pack + DLT: hypotheses and flags into ws (bestH / inlier / result untouched)
 *   rfx_ransac_degenerate_gather(ws, ...)          the flagged hypotheses that survived the duplicate filter, ascending per pair, and
 *                                                  the point coordinates of their samples, one row each (below)
 *   [host: LAPACK on exactly those systems -- what the reference itself computes on this host]
 *   rfx_ransac_patch_h_rows(ws, ..., H_rows)       re-solved homographies in, det gate re-evaluated
 *   rfx_ransac_h4_batched_stage(..., stages = 2)   count + select on the patched hypotheses
 * stages = 3 is rfx_ransac_h4_batched.  cap / N / batch / ws as for rfx_ransac_h4_batched (same workspace across the calls). */
int rfx_ransac_h4_batched_stage(const float* match1, const float* match2, const int32_t* n, int cap, const int64_t* samples,
                                int N, float tol, float* bestH, uint8_t* inlier, int32_t* result, void* ws, int batch,
                                int stages, void* stream);
/* The exchange (ABI 17: the only form; the (batch,kcap) lists of ABI 7-16 are gone).  rfx_ransac_degenerate_gather, after stage 1: lists the
 * flagged hypotheses of every pair (idx (batch,N) int32, count (batch) int32 -- device scratch), off (batch+1) int32 = exclusive
 * prefix of count with off[batch] = total (device; also stored to off_host when non-NULL), and writes ONE ROW PER FLAGGED
 * HYPOTHESIS at row off[b]+k of xy_rows: 16 floats = the sample's 4 source points (x, y) then its 4 target points (x, y), i.e.
 * X[:, :, :2] | Y[:, :, :2] of outil.Homography(X, Y) (utils/outil.py:68-71) -- the input rows of rfx_host_dlt_null_vectors
 * (rfx_host_api.h).  off_host and xy_rows may be PINNED HOST memory (hipHostMalloc / torch pin_memory: device-visible, coherent):
 * the kernels then store straight into it and the host reads it after ONE event wait, no copy.  Rows >= row_cap are dropped
 * (the caller compares off[batch] with row_cap, grows the buffer and calls again).
 * rfx_ransac_patch_h_rows: the re-solved homographies, row off[b]+k of H_rows (9 f32 per row; device or pinned host memory),
 * into the hypotheses idx[b][k]; det gate re-evaluated.  Then stage 2. */
int rfx_ransac_degenerate_gather(const void* ws, const float* match1, const float* match2, const int32_t* n, int cap,
                                 const int64_t* samples, int N, int batch, int32_t* idx, int32_t* count, int32_t* off,
                                 int32_t* off_host, float* xy_rows, int row_cap, void* stream);
int rfx_ransac_patch_h_rows(void* ws, int cap, int N, int batch, const int32_t* idx, const int32_t* count, const int32_t* off,
                            const float* H_rows, int row_cap, void* stream);
/* rfx_dlt4_homography + the per-system flag byte (bit0 set; bit1: det(H) > 1e-6; bit2 (4): rank deficient). */
int rfx_dlt4_homography_flags(const float* X, const float* Y, int N, float* Hout, uint8_t* flags, void* stream);

/* Match lists of a batch (quick_start/coarseAlignFeatMatch.py:150-155): match1[b,i] = (xa[idx1[b,i]], ya[idx1[b,i]], 1),
 * match2[b,i] = (xb[idx2[b,i]], yb[idx2[b,i]], 1) for i < n[b], zeros after.  idx1/idx2 (batch,cap) int64 as written by
 * rfx_mutual_nn_batched_f32; xa/ya = source cell coordinates (getWHTensor "H"/"W" of all scales, utils/outil.py:21-24),
 * xb/yb = target cell coordinates; match1/match2 (batch,cap,3). */
int rfx_gather_matches_f32(const int64_t* idx1, const int64_t* idx2, const int32_t* n, int cap, const float* xa,
                           const float* ya, const float* xb, const float* yb, float* match1, float* match2, int batch,
                           void* stream);

/* (ABI 11) The same for a ragged batch, pairs of different sizes (quick_start/coarseAlignFeatMatch.py:150-155 per pair): pair b's
 * cell coordinates are its own slice of packed tables, xa/ya + offA[b] and xb/yb + offB[b] (offA, offB: (batch) int64 element
 * offsets); idx1/idx2 (batch,cap) int64 as written by rfx_mutual_nn_ragged_f32; rows at or past n[b] are zero. */
int rfx_gather_matches_ragged_f32(const int64_t* idx1, const int64_t* idx2, const int32_t* n, int cap, const float* xa,
                                  const float* ya, const long long* offA, const float* xb, const float* yb, const long long* offB,
                                  float* match1, float* match2, int batch, void* stream);

/* ------------------------------------------------------------------------------------------
 * The rounds of the multi-homography drivers without host glue (evaluation/evalHpatch/evaluation.py:211-243,
 * evaluation/evalKITTI/evaluation.py:270-336).  All per-pair state (explained-region mask, homography count, cached match
 * list, result record) stays on the device; `active` (int32, n_active entries, NULL = identity) names the pairs of the batch
 * that still iterate, and every per-round array is indexed by the position k in that list.
 * ------------------------------------------------------------------------------------------ */
/* The RANSAC index draw on the device (utils/outil.py:120 draws torch.randint(0, nbMatch, (nbIter, nbPoint),
 * device=match1.device): on a GPU run the reference draws on the GPU).  samples (batch,N,4) int64;
 * samples[b,h,p] = word p of Philox4x32-10(counter = (h, id(b), stream_id lo, stream_id hi), key = (seed lo, seed hi))
 * modulo n[b] (torch's mapping of 32 random bits to a range below 2^32); n (batch) int32 ON THE DEVICE, n[b] <= 0 -> zeros.
 * id(b) = pair_ids[b] (batch int32 ON THE DEVICE: the caller's ABSOLUTE pair ids) or b when pair_ids is NULL.  With the
 * drivers' stream_id = (epoch << 32) | round, a pair's draws depend on (seed, its id, the round) only -- not on which other
 * pairs share the batch, are still active, or on how the stream is sharded over ranks.
 * No host value of nbMatch is needed: the draw is enqueued behind the kernel that produces the counts. */
int rfx_draw_samples_i64(const int32_t* n, int64_t* samples, int N, int batch, uint64_t seed, uint64_t stream_id,
                         const int32_t* pair_ids, void* stream);

/* (ABI 8) The keep map CoarseAlign.getCoarse of variants A / C multiplies the target features with before EVERY mutual matching
 * (quick_start/coarseAlignFeatMatch.py:136-143, evaluation/evalYFCC/coarseAlignFeatMatch.py:158-166), for the active pairs of a
 * batch: keep[k][cell] = 1.0 where (1 - fg) bilinear-resized (align_corners=False) to the (rt, ct) target feature map exceeds
 * 0.5, else 0.0; fg = ((mask + (1 - bg)) > 0.5) as in evaluation/evalYFCC/evaluation.py:239.  keep (n_active, rt*ct) is what
 * rfx_mutual_nn_batched_f32 takes as maskB -- the per-round re-matching of the YFCC driver shape stays on the device.
 * mask (batch,h,w) 0/1 floats or NULL together with bg == NULL (nothing explained, no background: all ones);
 * bg (batch,h,w) or NULL (= all ones); active (n_active) int32 or NULL (= 0..n_active-1). */
int rfx_keep_mask_f32(const float* mask, const float* bg, const int32_t* active, int n_active, int h, int w, int rt, int ct,
                      float* keep, void* stream);

/* CoarseAlign.getCoarse of the evaluation variant up to the match lists (evaluation/evalHpatch/coarseAlignFeatMatch.py:
 * 156-170) for the active pairs of a batch: fg = ((mask + (1 - bg)) > 0.5), MtExtend = 1 - fg bilinear-resized
 * (align_corners=False) to the (rt, ct) target feature map and thresholded at 0.5 -- evaluated only at the cells the cached
 * matches point to -- and the surviving matches compacted IN ORDER into match1/match2 (n_active,cap,3) as
 * rfx_gather_matches_f32 lays them out (rows >= n_out[k] zero); n_out (n_active) int32; kept (n_active,cap) int32 or NULL =
 * slot in the cached list of every surviving match (-1 padding).  idx1/idx2 (batch,cap) int64 + count (batch) int32 = the
 * cached mutual matches (rfx_mutual_nn_batched_f32); mask (batch,h,w) 0/1 floats; bg (batch,h,w) or NULL (= all ones). */
int rfx_filter_matches_f32(const int64_t* idx1, const int64_t* idx2, const int32_t* count, int cap, const int32_t* active,
                           int n_active, const float* mask, const float* bg, int h, int w, int rt, int ct, const float* xa,
                           const float* ya, const float* xb, const float* yb, float* match1, float* match2, int32_t* n_out,
                           int32_t* kept, void* stream);

/* The accept rule, mask update and result-record store of one round.  match (n_active,h,w) = PredFlowMask's matchability
 * (after the small-component filter for KITTI); mask (batch,h,w) in/out; ransac_result (n_active,4) from
 * rfx_ransac_h4_batched; n_match (n_active); nbH (batch) int32 in/out = homographies accepted so far.
 *   mode 0 (evalHpatch/evaluation.py:225,238-239): gain = mean(match * (1 - fg)); mask <- (mask + match * (1 - fg)) >= 1
 *   mode 1 (evalKITTI/evaluation.py:322,332-333):  gain = mean((match > 0.9999) * (1 - fg)); mask <- (... ) > 0.9999
 * accept[k] = n_match >= 4 && status == 0 && (gain > th || nbH == 0); gain is the float64 sum of the float32 terms divided by
 * h*w and rounded to float32 (numpy's float32 mean up to summation order).  For an accepted pair the record row
 * rec + b*rec_stride (floats; NULL = no records) receives, at slot s = nbH[b] < max_h: H -> [off_H + 9 s], flowDown8 (2,h8,w8)
 * -> [off_flow + 2 h8 w8 s], match12Down8 | match21Down8 -> [off_match + 2 h8 w8 s], flowD2 (2,hd2,wd2; NULL outside KITTI) ->
 * [off_d2 + 2 hd2 wd2 s], and element 0 = the new homography count; then nbH[b] += 1.  The host reads back `accept`
 * (n_active int32) -- the ONE device-to-host copy of a round.  ws: rfx_multih_accept_ws_bytes(n_active). */
size_t rfx_multih_accept_ws_bytes(int n_active);
int rfx_multih_accept_f32(const float* match, float* mask, const float* bg, const int32_t* active, int n_active, int h, int w,
                          const int32_t* ransac_result, const int32_t* n_match, int32_t* nbH, double th, int mode,
                          int32_t* accept, float* gain, void* ws, const float* bestH, const float* flowDown8,
                          const float* match12Down8, const float* match21Down8, int h8, int w8, const float* flowD2, int hd2,
                          int wd2, float* rec, long long rec_stride, int max_h, int off_H, int off_flow, int off_match,
                          int off_d2, void* stream);

/* (ABI 12) The two round kernels above for ACTIVE PAIRS OF DIFFERENT SIZES (a ragged batch; the loop of
 * evaluation/evalHpatch/evaluation.py:184-243 runs per pair, so a dataset of mixed image sizes is the normal case).  Per-pair state
 * is packed: pair b's explained-region mask (and background map) are h_b * w_b floats at element offset moff[b] (batch int64) of
 * ONE float buffer, and row b of the device table geom (batch,6) int32 holds its geometry: h, w (target image), rt, ct (target
 * feature map), h8, w8 (the /8 maps of the fine stage).  Each kernel runs the dense kernel's body on the pair's own values, so a
 * pair's outputs are bit for bit those of the dense entry point called on that pair alone.
 *
 * rfx_filter_matches_ragged_f32 (evaluation/evalHpatch/coarseAlignFeatMatch.py:156-170 per pair): idx1/idx2 (batch,cap) + count
 * as written by rfx_mutual_nn_ragged_f32; pair b's cell-coordinate tables are the slices xa/ya + offA[b], xb/yb + offB[b] of packed
 * tables (offA, offB: batch int64, as for rfx_gather_matches_ragged_f32); the resize scales are h_b / rt_b and w_b / ct_b rounded to
 * float32 exactly as rfx_filter_matches_f32 forms them.  Outputs as the dense kernel's: match1/match2 (n_active,cap,3), n_out
 * (n_active), kept (n_active,cap) or NULL -- what rfx_ransac_h4_batched and rfx_draw_samples_i64 consume. */
int rfx_filter_matches_ragged_f32(const int64_t* idx1, const int64_t* idx2, const int32_t* count, int cap, const int32_t* active,
                                  int n_active, const float* mask, const float* bg, const long long* moff, const int32_t* geom,
                                  const float* xa, const float* ya, const long long* offA, const float* xb, const float* yb,
                                  const long long* offB, float* match1, float* match2, int32_t* n_out, int32_t* kept,
                                  void* stream);

/* rfx_keep_mask_f32 for ACTIVE PAIRS OF DIFFERENT SIZES, one launch: the keep map variant C's getCoarse multiplies the target features
 * with before the mutual matching of EVERY round (evaluation/evalYFCC/coarseAlignFeatMatch.py:158-166).  mask / bg: the packed buffers
 * above (pair b's h_b * w_b floats at moff[b], geometry in geom[b]); bg NULL = all foreground; mask NULL = nothing explained yet (the
 * candidate search); both NULL = every cell kept.  For b = active[k] (k itself when active is NULL) the cell value is the one
 * rfx_keep_mask_f32 computes for that pair alone -- same interpolation, same operation order, scales h_b / rt_b and w_b / ct_b rounded
 * to float32 as the dense entry point forms them -- stored as 0.0 / 1.0 in keep[b * ldB + cell], cell < rt_b * ct_b: the pair's row
 * sits at its own position b, the layout rfx_mutual_nn_ragged_f32 reads its maskB in.  Columns from rt_b * ct_b on and the rows of
 * pairs that are not in the list are NOT written.  nB_round (batch int32, or NULL) receives rt_b * ct_b at the active pairs'
 * positions only; zeroed by the caller and passed to rfx_mutual_nn_ragged_f32 as nB, it makes the matching skip every other pair
 * (count 0, no work).  max_cells: the largest rt_b * ct_b among the active pairs, <= ldB; the grid is
 * (ceil(max_cells / 256), n_active) workgroups of 256 threads, n_active <= 65535 (RFX_E_LIMIT).  A pair whose table row is not
 * positive, or has more cells than ldB, gets no cell and nB_round 0. */
int rfx_keep_mask_ragged_f32(const float* mask, const float* bg, const long long* moff, const int32_t* geom, const int32_t* active,
                             int n_active, int ldB, int max_cells, float* keep, int32_t* nB_round, void* stream);

/* rfx_multih_accept_ragged_f32 (evalHpatch/evaluation.py:225,238-239; mode 1: evalKITTI/evaluation.py:322,332-333): the accept rule,
 * mask update and record store of rfx_multih_accept_f32.  The round's per-pair inputs are packed PER ACTIVE PAIR (offsets per k, the
 * order the fine stage of the round produced them in): match of pair k = h_b * w_b floats at match_off[k] (n_active int64);
 * flowDown8 of pair k at 2 * off8[k], match12Down8 / match21Down8 at off8[k] (n_active int64; required when one of the three
 * is given).  mask / bg are packed per PAIR (moff[b]).  gain: pair k's own HW is cut into the same 64 slices of ceil(HW / 64)
 * pixels, summed in the same order in double, as the dense kernel does for that pair.  max_hw = the largest h * w among the active
 * pairs (sizes the mask-update grid only).  Records: one row of rec_stride floats per pair, header and H slots as in the dense
 * layout (off_H, off_flow), flowDown8 slots of 2 h8_b w8_b floats from off_flow, matchDown8 slots from off_flow + 2 h8_b w8_b max_h
 * (rfx.ops.MultiHRecordsRagged); this entry point stores no flowD2 part (rfx_multih_accept_ragged_d2_f32 below does).
 * ws: rfx_multih_accept_ragged_ws_bytes(n_active). */
size_t rfx_multih_accept_ragged_ws_bytes(int n_active);
int rfx_multih_accept_ragged_f32(const float* match, const long long* match_off, float* mask, const float* bg,
                                 const long long* moff, const int32_t* geom, const int32_t* active, int n_active, long long max_hw,
                                 const int32_t* ransac_result, const int32_t* n_match, int32_t* nbH, double th, int mode,
                                 int32_t* accept, float* gain, void* ws, const float* bestH, const float* flowDown8,
                                 const float* match12Down8, const float* match21Down8, const long long* off8, float* rec,
                                 long long rec_stride, int max_h, int off_H, int off_flow, void* stream);

/* (ABI 14) rfx_multih_accept_ragged_f32 with the KITTI part of the record (evaluation/evalKITTI/evaluation.py:326: the half-resolution
 * /8 flow saved per homography): flowD2 of active pair k = 2 * hd2_b * wd2_b floats at element 2 * offd2[k] (n_active int64) of a
 * packed buffer, d2dims (batch,2) int32 = hd2_b, wd2_b per PAIR.  For an accepted pair slot s of its row also receives flowD2 at
 * off_flow + 4 h8_b w8_b max_h + 2 hd2_b wd2_b s -- where the dense row of that pair alone (MultiHRecords(1, h8, w8, hd2, wd2)) has
 * its off_d2.  flowD2, offd2 and d2dims are required; everything else is rfx_multih_accept_ragged_f32's. */
int rfx_multih_accept_ragged_d2_f32(const float* match, const long long* match_off, float* mask, const float* bg,
                                    const long long* moff, const int32_t* geom, const int32_t* active, int n_active,
                                    long long max_hw, const int32_t* ransac_result, const int32_t* n_match, int32_t* nbH, double th,
                                    int mode, int32_t* accept, float* gain, void* ws, const float* bestH, const float* flowDown8,
                                    const float* match12Down8, const float* match21Down8, const long long* off8,
                                    const float* flowD2, const long long* offd2, const int32_t* d2dims, float* rec,
                                    long long rec_stride, int max_h, int off_H, int off_flow, void* stream);

/* ------------------------------------------------------------------------------------------
 * rfx_conv1x1_split_f32 (ABI 10): the 1x1 / stride 1 / pad 0 convolution of rfx_conv2d_f32 (the Bottleneck conv1 / conv3 layers,
 * model/resnet50.py:71-79,93-103) with float32 results computed on the bf16 matrix cores by EXACT operand splitting:
 *     x = hi + mid + lo,  hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)      (round to nearest even; the sum is exact)
 *     out[n,m,p] = act(scale[m] * S + shift[m] + residual),
 *     S = sum_k (wh xh) + sum_k (wh xm + wm xh + wm xm + wh xl + wl xh)                 (every product exact in float32; the two
 *         sums in two float32 accumulators that round once per 16 k, added once at the end; the three dropped terms are below
 *         2^-24 (1 + 2^-10) |w x|, a bound nearly attained).  RMS error against the float64 sum: 0.4x the fp32 kernel's fma chain
 *         (profiles/r06_bf16_split_study.json); the max error at K >= 2304 is 1.2x - 2.9x the chunked fp32 kernels'
 *         (profiles/split_max_error_ratio.json).
 * NOT bit-identical to rfx_conv2d_f32 (closer to the exact sum in rms); +-inf inputs give NaN.  Cin % 16 == 0.
 * wS: the weights split on the host and packed in fragment order, bf16 bit patterns (uint16):
 *     wS[kb = k / 16][piece (hi, mid, lo)][h = (k % 16) / 8][m (Mpad = Cout rounded up to 128, rows >= Cout zero)][k % 8]
 * in (N,Cin,HW), out / residual (N,Cout,HW) float32.
 * ------------------------------------------------------------------------------------------ */
int rfx_conv1x1_split_f32(const float* in, const void* wS, const float* scale, const float* shift, const float* residual,
                          float* out, int N, int Cin, int HW, int Cout, int act, void* stream);
/* ... with a stride (1 or 2; pad 0): the projection shortcuts of the trunk (model/resnet50.py:139-143): out (N,Cout,Ho,Wo),
 * Ho = (Hin - 1) / stride + 1, reads input pixel (y * stride, x * stride). */
int rfx_conv1x1_split_strided_f32(const float* in, const void* wS, const float* scale, const float* shift, const float* residual,
                                  float* out, int N, int Cin, int Hin, int Win, int Cout, int stride, int act, void* stream);
/* Output channels per workgroup tile of the two launches above at N images of HWout OUTPUT pixels: 64 (Cout <= 64), 128, or 256 --
 * the 8-wavefront instance that stages a 128-pixel activation image once for 256 channels, taken where Cout >= 256, Cin >= 512 and
 * the launch's rounds over the CUs come out shorter than the 128-channel tile's (the measured rule in csrc/conv1x1s.hip).  Every
 * instance returns the same bits (same k order, same products, same epilogue).
 * RFX_C1S_WIDE (environment, read once): 0 = never 256; 1 = 256 wherever Cout >= 256. */
int rfx_conv1x1_split_tile_channels(int N, int Cin, int HWout, int Cout);
/* rfx_conv3x3_split_f32 (ABI 10): the same scheme for the 3x3 / stride 1 / pad 1 convolution (ResNet-50 layer3 conv2,
 * model/resnet50.py:75; the FeatureExtractor's BasicBlock convolutions, model/model.py:32-35; conv2 / conv3 of the NetFlowCoarse /
 * NetMatchability stacks, model/model.py:170-181): nine shifted 1x1 products over one staged, split halo patch.  Cin % 16 == 0.
 * wS3: bf16 bit patterns, [kb = c / 16][tap = kh * 3 + kw][piece][h = (c % 16) / 8][m (Mpad)][c % 8] = piece of W[m][c][kh][kw].
 * in (N,Cin,H,W), out / residual (N,Cout,H,W) float32.  NOT bit-identical to rfx_conv3x3_f32 / rfx_conv2d_f32 (closer to the exact sum in rms). */
int rfx_conv3x3_split_f32(const float* in, const void* wS3, const float* scale, const float* shift, const float* residual,
                          float* out, int N, int Cin, int H, int W, int Cout, int act, void* stream);
/* ... stride 2 (pad 1): ResNet-50 layer2.0 / layer3.0 conv2 (model/resnet50.py:75), the FeatureExtractor's strided conv1
 * (model/model.py:32).  out (N,Cout,Ho,Wo), Ho = (H - 1) / 2 + 1; same wS3; Cin % 16 == 0; 128-channel tiles. */
int rfx_conv3x3_split_s2_f32(const float* in, const void* wS3, const float* scale, const float* shift, const float* residual,
                             float* out, int N, int Cin, int H, int W, int Cout, int act, void* stream);

/* ------------------------------------------------------------------------------------------
 * rfx_conv1x1_expand64_f32 (ABI 15): the 1x1 / stride 1 / pad 0 convolution of rfx_conv2d_f32 for Cin = 64 and Cout = 256 (the
 * 64 -> 256 expansions of ResNet-50 layer1, model/resnet50.py:77-79) as a kernel of its own (csrc/conv1x1e.hip): the whole weight
 * matrix stays in LDS for the life of a persistent workgroup, a wavefront produces every output channel of its 32 pixels from
 * operands it loads once.
 *     out[n,m,p] = act(fmaf(sum_k in[n,k,p] * w[m,k], scale[m], shift[m]) + residual[n,m,p])
 * Same k pairs in the same ascending order, one fma chain per output, same epilogue: BIT-IDENTICAL to rfx_conv2d_f32 on this geometry.
 * wT: rfx_conv2d_f32's pack of the (Cout, 64, 1, 1) weight (wT[k][Mpad], Mpad = Cout here); scale / shift (Cout) or NULL (1 / 0);
 * residual (N,Cout,HW) or NULL; act = RFX_ACT_NONE or RFX_ACT_RELU.  in (N,64,HW), out (N,Cout,HW) float32, any HW.
 * Launch: min(CUs, ceil(T / 8)) workgroups of 8 wavefronts, T = ceil(N * HW / 32) pixel tiles; wavefront w of workgroup g walks the
 * tiles 8 g + w, 8 g + w + 8 * workgroups, ...
 * Returns RFX_E_ARG for Cin != 64, stride != 1, Cout % 256 != 0, another activation, or while a grouped launch records
 * (rfx_group_begin: the group keeps rfx_conv2d_f32's launches); RFX_E_LIMIT for Cout > 256.
 * ------------------------------------------------------------------------------------------ */
int rfx_conv1x1_expand64_f32(const float* in, const float* wT, const float* scale, const float* shift, const float* residual,
                             float* out, int N, int Cin, int HW, int Cout, int stride, int act, void* stream);
/* ... two-source form: a Bottleneck's conv3 and its projection shortcut in one launch (model/resnet50.py:93-103 with :139-143),
 *     d   = fmaf(sum_k in_b[n,k,p] * w_b[m,k], scale_b[m], shift_b[m])                  (rounded to float32)
 *     out = relu(fmaf(sum_k in_a[n,k,p] * w_a[m,k], scale_a[m], shift_a[m]) + d)
 * -- the operations, in their order, of rfx_conv2d_f32(in_b, ..., RFX_ACT_NONE) followed by rfx_conv2d_f32(in_a, ..., residual = d,
 * RFX_ACT_RELU): bit-identical to that pair, and d never goes to memory.  in_a, in_b (N,64,HW) over the same pixels; both weight
 * sets as above, both with Cin = 64; errors as above. */
int rfx_conv1x1_expand64_dual_f32(const float* in_a, const float* wT_a, const float* scale_a, const float* shift_a,
                                  const float* in_b, const float* wT_b, const float* scale_b, const float* shift_b, float* out,
                                  int N, int Cin, int HW, int Cout, int stride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sky segmentation forward pass: SegNet.getSky (segNet/segEval.py:23-43) = ResNet-50-dilated encoder
 * (segNet/segModel.py:156-215: layer3 / layer4 with dilation 2 / 4 instead of stride) + PPM decoder (:218-265) over five
 * scales, averaged, arg-max, (pred == segId).  Called once per target image by CoarseAlign.skyFromSeg
 * (evaluation/evalHpatch/coarseAlignFeatMatch.py:63-64,152-153; evaluation/evalHpatch/evaluation.py:177-180).
 * The convolutions run on the convolution family above plus ONE more geometry:
 *
 * rfx_conv2d_dilated_f32: rfx_conv2d_f32 with `dilation` > 1 (segModel.py:196-205: 3x3, dilation = padding = 2 or 4):
 *     out[n,m,oh,ow] = act(scale[m] * sum in[n,c,oh*s-p+kh*d,ow*s-p+kw*d] * w[m,c,kh,kw] + shift[m] + residual)
 * wT as for rfx_conv2d_f32; ktab holds the DILATED offsets: (c<<8)|((kh*d)<<4)|(kw*d), (KH-1)*d + 1 <= 15.  Same kernels, same
 * summation order as rfx_conv2d_f32 (the gather adds the table's offsets to the window origin as they are).
 * ------------------------------------------------------------------------------------------ */
int rfx_conv2d_dilated_f32(const float* in, const float* wT, const int32_t* ktab, const float* scale,
                           const float* shift, const float* residual, float* out, int N, int Cin, int Hin,
                           int Win, int Cout, int KH, int KW, int stride, int pad, int dilation, int act, void* stream);
/* nn.AdaptiveAvgPool2d((Hout, Wout)) on NC planes (segModel.py:227): window [floor(o*In/Out), ceil((o+1)*In/Out)), row-major sum / count. */
int rfx_adaptive_avgpool2d_f32(const float* in, float* out, int NC, int Hin, int Win, int Hout, int Wout, void* stream);
/* scores[n,c,p] = (accumulate ? scores[n,c,p] : 0) + softmax_c(logits[n,:,p]) / div      (segModel.py:258 + segEval.py:34-35:
 * ``scores = scores + pred_tmp / 5``); logits / scores (N,C,HW). */
int rfx_softmax_accum_f32(const float* logits, float* scores, int N, int C, long long HW, float div, int accumulate, void* stream);
/* torch.max(scores, dim=1) -> mask[n,p] = (pred == id) (complement != 0: 1 - that), float32 (segEval.py:37-43); pred (N,HW) int32
 * optional (NULL: not stored).  First maximum wins. */
int rfx_argmax_mask_f32(const float* scores, int N, int C, long long HW, int id, int complement, float* mask, int32_t* pred,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Sky masks for a batch of targets (ADDED under ABI 17: no existing entry point moved).
 * ------------------------------------------------------------------------------------------ */
/* segNet/segEval.py:27-43 after the network passes, in ONE kernel: per scale s = 0..S-1 in order
 *     rfx_resize_bilinear_f32(logits[s], align_corners = 0) to (H, W) -> rfx_softmax_accum_f32(div) (scale 0 stores, the others add),
 * then rfx_argmax_mask_f32(id, complement) -- bit for bit that chain's pred and mask, without the (N,C,H,W) up-sampled logits and
 * scores: one thread per output pixel forms the taps of every scale once, then per scale the maximum and the sum of expf(v - mx)
 * over the classes in class order, then ((p_0 + p_1) + ...) with p_s = expf(v - mx_s) / sum_s / div per class and the running
 * first maximum (strict >, NaN wins like torch.max).  logits: HOST array of S device pointers, map s is (N, C, hs[s], ws[s])
 * float32; hs, ws: HOST arrays; all three are read during the call and travel in the kernel's argument block.  mask (N,H,W) float32,
 * pred (N,H,W) int32 or NULL.  Records inside a grouped launch like the other pointwise families.
 * RFX_E_ARG: a null pointer other than pred, S outside 1..8, a non-positive size or div.  RFX_E_LIMIT: N*H*W or an hs[s]*ws[s]
 * above 2^31 - 1.  All of these are checked before any HIP call. */
int rfx_seg_vote_f32(const float* const* logits, const int32_t* hs, const int32_t* ws, int S, int N, int C, int H, int W, float div,
                     int id, int complement, float* mask, int32_t* pred, void* stream);

/* The byte image scipy.misc.imresize makes of a sky mask before it resizes it, turned k quarter turns
 * (evaluation/evalYFCC/evaluation.py:193,200,212: np.rot90(It_bg, k), then imresize -> scipy 1.2.3 pilutil.bytescale; k = 0 for
 * evalHpatch/evaluation.py:180, evalCorr/evaluation.py:187, evalKITTI/evaluation.py:247-248).  mask (N,H,W) float32 of 0 / 1 values:
 * a pixel becomes 255 where the mask is non-zero, provided ITS map holds both a zero and a non-zero value; a constant map becomes all
 * zeros (bytescale's cscale = (cmax - cmin) or 1).  out (N,Ho,Wo) bytes = np.rot90(bytes, k), (Ho, Wo) = (H, W) for even k and (W, H)
 * for odd k.  ws: rfx_sky_bytes_ws_bytes(N) bytes = one flag word per map, zeroed by the call; only ORs of constants reach a word, so
 * no result depends on the order in which workgroups run.  Three stream-ordered operations.
 * RFX_E_ARG: a null pointer, a non-positive N, H or W, k outside 0..3.  RFX_E_LIMIT: N*H*W > 2^31 - 1. */
size_t rfx_sky_bytes_ws_bytes(int N);
int rfx_sky_bytes_u8(const float* mask, int N, int H, int W, int k, uint8_t* out, void* ws, void* stream);
/* out[i] = in[i] < threshold ? 1.0f : 0.0f -- the scripts' ``(imresize(It_bg, (Ith, Itw)) < 128).astype(np.float32)``
 * (evalHpatch/evaluation.py:180) on the resized bytes.  RFX_E_ARG: a null pointer or total <= 0. */
int rfx_less_than_u8_f32(const uint8_t* in, long long total, int threshold, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Aligned source images of a batch (both ADDED under ABI 17: no existing entry point moved).
 * ------------------------------------------------------------------------------------------ */
/* quick_start/align2images.py:97-98,117 (F.grid_sample(IsTensor, flow12), ToPILImage, fine_aligned_source.png) and :25-28,112
 * (get_Avg_Image, the 50 % overlay with the target) for EVERY pair of a batch, as uint8 HWC images, in one launch each.
 *
 * rfx_warp_records_u8: from the drivers' records.  rec, rec_elems, width, max_h, off_H, off_flow, table (B,8), B, max_hw, th, multiH,
 * cycle, bg, total_px: as rfx_assemble_records_f32 takes them, with the same row checks (records with a flowD2 part, the KITTI
 * drivers', are not covered: their flow goes through rfx_warp_flow_u8).  itable (B,4) int64 on the device, row b:
 *     address of the pair's source (Hs,Ws,3) uint8 | Hs | Ws | address of its target (H,W,3) uint8 at the OUTPUT size, or 0
 * so that sources of any sizes are read where they lie.  Outputs in the packed layout of the table's pixel offsets:
 * img (total_px,3) uint8; overlay (total_px,3) uint8 or NULL; mask (total_px) uint8 or NULL.  Per pixel of pair b:
 *     (fx, fy), found = flowGlobal and the explained bit of rfx_assemble_records_f32 at the pixel, from the record alone;
 *     per channel v = 0, then for each corner of ATen's bilinear sample of the SOURCE (zeros padding, align_corners = 0) that lies
 *     inside it, in the order nw, ne, sw, se: v = fma(float(byte) / 255.0f, weight, v) -- rfx_u8_to_f32_chw's x / 255 followed by
 *     rfx_grid_sample_f32, bit for bit;
 *     img = (uint8)(clamp(v, 0, 1) * 255.0f), the product rounded to float32, then truncated (mul(255).byte());
 *     overlay = (img + target) >> 1 per channel, where the pair has a target (a pair with target 0 leaves its overlay bytes alone);
 *     mask = 255 where found && (bg == NULL || bg[pixel] != 0), else 0  (binary of rfx_assemble_records_f32).
 * A NaN flow has no in-image corner: the pixel is 0.  A pair with nbH < 1 has the zero flow: every pixel samples the source's centre.
 * A table row that is refused, or an itable row without a source (address 0) or with a size that is not positive or whose Hs*Ws
 * leaves int32, is skipped: nothing of it is read or written.  One thread per pixel stores its own bytes; no LDS, no atomics, no
 * workgroup waits on another; blockIdx.y = the pair, the grid over a pair's pixels is capped at 8192 workgroups and strides.
 * RFX_E_ARG: a null rec, table, itable or img, a non-positive B, width, max_h or max_hw, offsets that do not describe a record,
 * rec_elems < B * width, total_px < max_hw, a table not 8-byte aligned.  RFX_E_LIMIT: B > 65535, max_hw > 2^31 - 1.
 *
 * rfx_warp_flow_u8: the same image tail on a stored flow (total_px,2) float32 in the packed layout -- what
 * rfx_assemble_records_f32 / rfx_assemble_kitti_records_f32 fill, or quick-start's flow12 (B = 1).  table (B,8): only columns 4..6
 * (H | W | pixel offset) are read; binary (total_px) bytes or NULL is passed through to mask (255 where non-zero).
 * RFX_E_ARG: a null flow, table, itable or img, a mask without binary, a non-positive B or max_hw, total_px < max_hw, flow or a table
 * not 8-byte aligned.  RFX_E_LIMIT as above.  All of these are checked before any HIP call. */
int rfx_warp_records_u8(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow, const long long* table,
                        int B, long long max_hw, float th, int multiH, int cycle, const uint8_t* bg, const long long* itable,
                        uint8_t* img, uint8_t* overlay, uint8_t* mask, long long total_px, void* stream);
int rfx_warp_flow_u8(const float* flow, const long long* table, int B, long long max_hw, const uint8_t* binary, const long long* itable,
                     uint8_t* img, uint8_t* overlay, uint8_t* mask, long long total_px, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RFX_API_H */
