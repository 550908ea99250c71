/* ape_hip.h -- C ABI of libape_hip.so, the MI355X (gfx950) hot path behind the Python call signatures of
 * KochPJ/AutoPoseEstimation's seg -> DenseFusion -> ICP slice.
 *
 * Conventions ("Ownership / errors / threading"):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - the caller owns every buffer, nothing is allocated behind its back (workspaces are passed in);
 *   - every entry point enqueues on the hipStream_t passed as `void* stream` (NULL = default stream)
 *     and returns without synchronising;  it is re-entrant per stream;
 *   - return value: APE_OK (0) or a negative APE_E* code; nothing throws, nothing prints.
 *
 * Each entry names the reference interface it replaces (file:line relative to the reference repo).
 * The Python side (autoposeestimation_amd/_lib.py) binds exactly these symbols with ctypes;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 */
#ifndef APE_HIP_H
#define APE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#define APE_STATIC_ASSERT static_assert
#else
#define APE_STATIC_ASSERT _Static_assert
#endif

#define APE_OK 0
#define APE_EINVAL (-1)   /* bad shape / unsupported parameter combination */
#define APE_ELAUNCH (-2)  /* hipGetLastError() != hipSuccess after the launch */
#define APE_EWORKSPACE (-3) /* workspace too small */

/* ABI version: bumped whenever a signature below changes. */
int ape_abi_version(void);
/* Name of the last HIP error seen by this thread's failing call (static storage). */
const char* ape_last_error(void);

/* ---- k-NN -------------------------------------------------------------------------------------------
 * Replaces `int knn(at::Tensor& ref, at::Tensor& query, at::Tensor& idx)`
 *   DenseFusion/lib/knn/src/knn.h:12-66 (dispatcher), src/cpu/knn_cpu.cpp:4-55 (semantics),
 *   src/cuda/knn.cu:217-263 (the CUDA path this supersedes), bound at src/vision.cpp:3-5.
 * ref[batch][dim][ref_nb] f32, query[batch][dim][query_nb] f32 (contiguous, as knn.h:23-24 assumes),
 * idx[batch][k][query_nb] i64, filled with 1-BASED ref indices of the k smallest squared-L2 distances
 * in ascending order, ties in ascending ref index (knn_cpu.cpp:30 swaps only on '>').
 * Distances are accumulated in float32 dimension by dimension, one rounding per multiply and add
 * (no FMA), so indices are bit-identical to the reference CPU build.
 * Returns APE_OK (the reference returns 1; the Python wrapper keeps that convention). */
int ape_knn_f32(const float* ref, const float* query, int64_t* idx,
                int batch, int dim, int ref_nb, int query_nb, int k, void* stream);

/* ---- dense contractions: conv2d / 1x1 / Linear, exact fp32 on the matrix cores ---------------------------
 * One entry point replaces every torch.nn.Conv2d / Conv1d(k=1) / Linear forward on the path:
 *   DenseFusion/lib/extractors.py:14-16,82-89,101-105 (ResNet convs), pspnet.py:12-17,30-33,53-55 (PSP, up-convs,
 *   final 1x1), network.py:42-49,76-92,139-146,175-182 (PointNet / head 1x1 chains, refiner Linear stacks),
 * with the following pointwise op fused: bias, residual add (extractors.py:40), ReLU / PReLU / sigmoid.
 *
 * Layouts: x[B][H][W][ldx] f32 (NHWC, the layer reads channels xoff .. xoff+Cin-1), w[Cout][KH][KW][Cin] f32,
 * y[B][Ho][Wo][ldy] (writes channels yoff .. yoff+Cout-1), residual like y with (ldr, roff).
 * bias: NULL, or bias[Cout] (bias_bstride = 0), or per-image bias[B][bias_bstride] (first Cout entries used).
 * Constraints: Cin, ldx, xoff multiples of 4 (16-byte loads); Ho/Wo must equal the conv arithmetic result. */
enum { APE_ACT_NONE = 0, APE_ACT_RELU = 1, APE_ACT_PRELU = 2, APE_ACT_SIGMOID = 3 };
typedef struct ape_conv_params {
    int32_t B, H, W, Cin, ldx, xoff;
    int32_t Ho, Wo, Cout, ldy, yoff;
    int32_t KH, KW, stride, pad, dil;
    int32_t act;            /* APE_ACT_* */
    float alpha;            /* PReLU slope (pspnet.py:33, single parameter) */
    int32_t bias_bstride;
    int32_t ldr, roff;
    int32_t ups;            /* 1: x is the LOW-resolution tensor [B][H/2][W/2][ldx] and the conv reads its bilinear x2
                               (align_corners=True) up-sampling on the fly (nn.Upsample + Conv2d of pspnet.py:30-32 fused);
                               only ape_conv3x3_halo_bf16 accepts it (H, W even), everything else requires 0 */
} ape_conv_params;
int ape_conv2d_nhwc_f32(const float* x, const float* w, const float* bias, const float* residual, float* y,
                        const ape_conv_params* params_host, void* stream);

/* ---- the same contraction on the bf16 matrix cores (fp32 accumulate, fp32 activations in HBM) ------------------
 * nsplit = 3: split-bf16 operands (x = hi + lo, three MFMA products per term, ~2^-16 relative operand error);
 * nsplit = 1: plain bf16 operands.  Same params / fused epilogue / layouts as ape_conv2d_nhwc_f32, except that the
 * weights are the packed planes produced by ape_pack_weights_bf16 from w[Cout][KH*KW*Cin] f32:
 * hi plane [Cout][Kp] bf16 then lo plane [Cout][Kp], Kp = K rounded up to 8 (ape_packed_weights_bf16_elems elements). */
long ape_packed_weights_bf16_elems(int cout, int K);
int ape_pack_weights_bf16(const float* w, void* out, int cout, int K, void* stream);
int ape_conv2d_nhwc_bf16(const float* x, const void* w_packed, const float* bias, const float* residual, float* y,
                         const ape_conv_params* params_host, int nsplit, void* stream);
/* Cin % 32 == 0 successor of ape_conv2d_nhwc_bf16 (same arguments, packed weights, numerics class and fused epilogue):
 * 16x16x32 MFMA, swizzled double-buffered LDS stages, register staging that writes tile t+1 after the barrier and re-issues
 * tile t+2 at once.  Takes every 1x1 conv / Conv1d(k=1) / Linear of the path (pspnet.py:12-17,53, network.py:42-49,76-92,
 * 139-146,175-182) and the k x k convs the LDS-halo kernel leaves.  variant: 0 = block shape chosen from (M, Cout, K),
 * 1 = 256x256, 2 = 128x128, 3 = 256x64, 4 = 256x192 (tuning aid).  ape_conv_gemm_supported(params) says whether it applies. */
int ape_conv_gemm_supported(const ape_conv_params* params_host);
int ape_conv_gemm_bf16(const float* x, const void* w_packed, const float* bias, const float* residual, float* y,
                       const ape_conv_params* params_host, int nsplit, int variant, void* stream);
/* ---- pre-split ("S32") activations --------------------------------------------------------------------------------------
 * The split-bf16 operands of the bf16 kernels above, made ONCE by the producing kernel's epilogue instead of by every consumer
 * tile: a pixel's C channels (C % 32 == 0) are C/32 groups of 128 bytes [hi: 32 x bf16 | lo: 32 x bf16], hi = bf16(v),
 * lo = bf16(v - hi) -- 4 bytes per channel, so (ld, offset) arithmetic in channels is unchanged.  Weights for S32 consumers use
 * the same grouping along K ("S32K": [Cout][K/32][hi 32 | lo 32], ape_pack_weights_s32k from w[Cout][K] f32).
 * ape_conv_gemm_s32: the 1x1 / stride-1 layers (pspnet.py:12-17,22-24 and the low-resolution channel mixing of :27-37) with
 * x in S32, operands streamed HBM -> LDS by LDS-DMA (no staging registers, no split VALU), y and the residual in either format.
 * Needs Cin % 32 == 0, ldx % 32 == 0, xoff % 32 == 0, Cout >= 128 and % 4; ape_conv_gemm_s32_supported(params) says so. */
enum { APE_FMT_F32 = 0, APE_FMT_S32 = 1 };
int ape_pack_weights_s32k(const float* w, void* out, int cout, int K, void* stream);
/* x[rows][C] f32 -> y[rows][C] S32 (to_s32 = 1) or back (to_s32 = 0: hi + lo); C % 32 == 0.  Tests and format boundaries only. */
int ape_convert_s32(const void* x, void* y, long rows, int C, int to_s32, void* stream);
int ape_conv_gemm_s32_supported(const ape_conv_params* params_host);
int ape_conv3x3_halo_s32_debug(int bits);   /* development aid, results unchanged by any bit: 1 = a static wave priority for waves 4-7 (lockstep kernel); 2 = one workgroup per tile; 8 = one channel tile per XCD (weights L2-resident, halos fetched n_tiles times: DESIGN.md 6f); 16 = four rows per wave-row group in every tile; 4096 = launch the lockstep (one-barrier, in-phase) kernel of rounds 2-5 instead of the ping-pong one (tools/mb_halo_pp.py, tests/test_gpu_s32.py) */
int ape_conv_gemm_s32_debug(int bits);   /* development aid: 16 / 32 / 64 / 8192 leave the results unchanged (k-tile rotation, no static priority, one tile per workgroup, 8192 = launch the ping-pong kernels: bit-identical, slower, tools/mb_gemm_pp.py); the ablation build (make ablations) also knows timing-only bits that break the results */
int ape_conv_gemm_s32(const void* x_s32, const void* w_s32k, const float* bias, const void* residual, int res_fmt, void* y,
                      int out_fmt, const ape_conv_params* params_host, void* stream);
/* The same contraction with PER-IMAGE weights: image i of the batch (params->H * params->W rows) multiplies with the S32K matrix at
 * w_s32k + i * w_image_stride_bytes (a multiple of 16), and no 256-row tile holds rows of two images.  No residual operand.
 * Used by the PSP module (DenseFusion/lib/pspnet.py:12-24), whose prior sum is folded into the bottleneck's contraction:
 * ape_psp_fold_operands builds both operands' extra 64 K-columns -- channels [Cin, Cin + 64) of every pixel of x_s32 (ld >= Cin + 64
 * channels per pixel) get the pixel's bilinear (align_corners = False) coefficients of the 1 + 4 + 9 + 36 prior cells, and
 * w_out[B][Cout][Cin/32 + 2 groups] gets the shared weights wf_s32k[Cout][Cin/32 groups] followed by frame b's prior values
 * z_s[b][cell][co] (z1..z6: the merged stage x bottleneck-column convs of the pooled maps, fp32 [B][s][s][Cout]) -- so that
 *     relu(W_f . f + sum_s upsample(Z_s) + bias)  ==  ape_conv_gemm_s32_per_image over K = Cin + 64
 * and the 4 * B * h * w * Cout-byte prior-sum tensor (ape_psp_prior_sum_f32) is neither written nor read back. */
int ape_conv_gemm_s32_per_image(const void* x_s32, const void* w_s32k, long w_image_stride_bytes, const float* bias, void* y, int out_fmt,
                                const ape_conv_params* params_host, void* stream);
int ape_psp_fold_operands(const void* wf_s32k, const float* z1, const float* z2, const float* z3, const float* z6, void* w_out, void* x_s32,
                          int B, int h, int w, int ld, int Cin, int Cout, void* stream);
/* ---- the point-feature front of the pose networks in one launch ----------------------------------------------------------------
 * Replaces PoseNetFeat / PoseRefineNetFeat up to the concatenation (DenseFusion/lib/network.py:39-68,136-168): with ReLU after every layer
 *   pf[m] = [conv1(x4[m]) 64 | e_conv1(emb[m]) 64 | conv2(conv1 out) 128 | e_conv2(e_conv1 out) 128],  x4[M][4], emb[M][32] f32,
 * the weights as ape_pack_weights_bf16 packs them (conv1 from w[64][4], e_conv1 [64][32], conv2 / e_conv2 [128][64]) and the biases.
 * Outputs, each optional (NULL = not written, at least one): pf[M][384] f32 and pf_s32, the same rows in the S32 layout.  parts selects
 * the x half (conv1, conv2: columns 0..63, 128..255) and / or the emb half (e_conv1, e_conv2: 64..127, 256..383); the columns and operands
 * of an unselected half are neither read nor written.  nsplit must be 3.  Every fp32 value and every S32 byte equals what
 * ape_conv2d_nhwc_bf16 (conv1), ape_conv_gemm_bf16 (the other three) and ape_convert_s32 give in five launches. */
enum { APE_POINT_FEAT_X = 1, APE_POINT_FEAT_EMB = 2 };
int ape_point_feat_bf16(const float* x4, const float* emb, const void* w_conv1, const float* b_conv1, const void* w_e_conv1,
                        const float* b_e_conv1, const void* w_conv2, const float* b_conv2, const void* w_e_conv2, const float* b_e_conv2,
                        float* pf, void* pf_s32, long M, int parts, int nsplit, void* stream);
/* Format-aware forms of three fp32 operations, for the tensors that cross between fp32 and S32 kernels: ape_conv_gemm_bf16 with the
 * OUTPUT in either format (the stride-2 convs that feed the first S32 3x3 layer), the multi-size adaptive average pool with the INPUT
 * in either format (ape_adaptive_avgpool_multi_nhwc_ld: the PSP pools of the S32 layer-4 map), ape_upconv3x3_gather_f32 with the OUTPUT
 * in either format (ape_upconv3x3_gather_ex: up_1's result feeds up_2's S32 channel mixing). */
int ape_conv_gemm_bf16_fmt(const float* x, const void* w_packed, const float* bias, const float* residual, void* y, int out_fmt,
                           const ape_conv_params* params_host, int nsplit, int variant, void* stream);
/* (variant, of both entry points: 0 = chosen from the shape, 1..6 a block shape of conv_gemm_kernel, 7 = conv_rows_kernel, the small-M form of
 * the pure 1x1 / stride-1 convolution with fp32 output and no residual -- APE_EINVAL for anything else -- which variant 0 takes up to 128
 * rows; 0 | 0x100 = variant 0 without that form.  Every variant forms the same sum per output element: same results bit for bit.) */
/* The PSP module's stage convolutions (pspnet.py:15-18, 22: `stage(feats) for stage in self.stages` -- four bias-free 1x1 convolutions of the
 * 1x1 / 2x2 / 3x3 / 6x6 pooled maps) are independent problems of 1 .. 18 tiles each: n <= 4 such 1x1 / stride-1 convolutions (fp32 in, fp32 out,
 * no residual) in ONE launch.  Problem i multiplies x[i] by w_packed[i] (ape_pack_weights_bf16 layout) under params_host[i]; bias may be NULL
 * or hold NULL entries.  Every output element is bit for bit what ape_conv_gemm_bf16 gives for that problem alone. */
int ape_conv_gemm_bf16_multi(int n, const float* const* x, const void* const* w_packed, const float* const* bias, float* const* y,
                             const ape_conv_params* params_host, int nsplit, void* stream);
/* Split-K form for the training tape's batch-1 layers (train.py:205-238 runs ONE 160x160 crop per step: its 20 x 20 feature maps are 4
 * row tiles of the 128 x 128 block, K up to 4608): the k-tiles are dealt to several workgroups per output tile, raw sums go to the
 * workspace, a second pass adds them in a fixed order with bias / residual / activation.  Same products, another summation order than
 * ape_conv_gemm_bf16; the inference path never takes it.  ..._workspace_bytes returns 0 when the shape is not worth splitting. */
size_t ape_conv_gemm_splitk_workspace_bytes(const ape_conv_params* params);
int ape_conv_gemm_bf16_splitk(const float* x, const void* w_packed, const float* bias, const float* residual, float* y,
                              const ape_conv_params* params, int nsplit, void* workspace, size_t workspace_bytes, void* stream);
/* The multi-size adaptive average pool (documented with ape_adaptive_avgpool_multi_workspace_bytes below) of x in either activation
 * format (APE_FMT_S32: C % 32 == 0 and ldx % 32 == 0), over the first C channels of a map that holds ldx >= C channels per pixel (the PSP
 * module's feature map with the 64 spare channels of ape_psp_fold_operands behind its 512: pspnet.py:15 pools the 512); outputs
 * [B,s,s,C] fp32.  in_fmt | APE_POOL_ATOM_ROWS: pass 1 with one workgroup per atom ROW instead of one per atom (the former kernel, kept
 * for A/B: same results bit for bit) */
enum { APE_POOL_ATOM_ROWS = 0x100 };
int ape_adaptive_avgpool_multi_nhwc_ld(const void* x, int in_fmt, float* const* ys_host, const int* sizes_host, int nsizes, int B, int H, int W,
                                       int C, int ldx, void* workspace, size_t workspace_bytes, void* stream);
/* ape_upconv3x3_gather_f32 with the OUTPUT in either activation format (APE_FMT_S32: C % 32 == 0) and the interpolation arithmetic
 * chosen: fma = 0 separately rounded products like ape_bilinear_nhwc_f32 (what ape_upconv3x3_gather_f32 uses), fma = 1 chained fused
 * multiply-adds acc = fma(l1, v1, fma(l0, v0, acc)) -- the unfused twin of ape_upconv3x3_fused_* called with fma = 1 */
int ape_upconv3x3_gather_ex(const float* z, const float* bias, void* out, int out_fmt, int B, int h, int w, int C, int act, float alpha,
                            int fma, void* stream);
/* Channel counts that are multiples of 64 take a second kernel with the same arithmetic (bit-identical outputs): strips of `rows` output
 * rows per workgroup, the z rows of every tap held in registers while the strip moves down (each z element is loaded ~1.2x instead of
 * ~5x).  rows >= 1 sets the strip height (default 30), 0 routes every call to the one-row kernel, < 0 only queries; returns the
 * previous value.  A process-wide tuning / test switch, not per stream. */
int ape_upconv3x3_gather_strip_rows(int rows);
/* PSPUpsample with 64 output channels (DenseFusion/lib/pspnet.py:27-37: nn.Upsample x2 align_corners=True -> Conv2d 3x3 pad 1 -> PReLU;
 * up_2 and up_3 of pspnet.py:50-51) as ONE kernel on an S32 input x[B][h][w][Cin] (Cin = 64): the low-resolution channel mixing
 * z = W9 . x (W9 S32K [9*64][Cin], row = tap*64 + co, as ape_upconv3x3_gather_f32 expects) runs on the matrix cores for the 10 x 16
 * low-resolution pixels under a 16 x 24 output tile, the row interpolation + tap-row sum happen on the accumulators (a lane holds one
 * low-resolution column in all rows), the column interpolation + tap-column sum through LDS; the 9*64-channel tensor z never exists
 * in memory.  Values are bit for bit those of ape_conv_gemm_s32 (z) followed by ape_upconv3x3_gather_ex(fma) on the same operands.
 * ..._fused_s32 writes out[B][2h][2w][64] in out_fmt; ..._fused_seghead_s32 feeds the pixels straight into the segmentation head
 * (ape_seg_head_f32: final 1x1 conv rows 0..C-1 + softmax(+softmax) + arg-max, pspnet.py:53-55, pipeline/utils.py:429-435) and writes
 * label[B][2h][2w] u8 / score f32 only.  ..._supported: 1 when the geometry is served (Cin == 64, Cout == 64, and the floor pattern of the
 * align_corners source index that the register form relies on holds for h and w; always true for the sizes of the reference). */
int ape_upconv3x3_fused_supported(int h, int w, int Cin, int Cout);
int ape_upconv3x3_fused_stamps(void* device_buffer);   /* diagnostic build (make stamps) only: [workgroups][12 waves][16] u64 cycle sums; NULL = off */
int ape_upconv3x3_fused_debug(int bits);    /* timing-only ablations for tools/mb_upfuse.py (0 = off; anything else gives WRONG results) */
int ape_upconv3x3_fused_s32(const void* x_s32, const void* w9_s32k, const float* bias, void* out, int out_fmt, int B, int h, int w, int Cin,
                            int act, float alpha, int fma, void* stream);
int ape_upconv3x3_fused_seghead_s32(const void* x_s32, const void* w9_s32k, const float* bias, int B, int h, int w, int Cin, int act, float alpha,
                                    int fma, const float* head_w, const float* head_b, int C, uint8_t* label, float* score, int double_softmax,
                                    void* stream);
/* 3x3 / stride 1 / pad == dilation in {1,2,4} convolutions with Cout >= 128 on S32 activations (extractors.py:29-43 blocks of layers
 * 2-4): the LDS-halo kernel with the halo rows and the weight tiles streamed by LDS-DMA into rings and every fragment read
 * prefetched one tap ahead.  Same accumulators as ape_conv3x3_halo_bf16(nsplit = 3) on the fp32 form of x; weights S32K in the
 * (tap, channel) K order of the packed layout; y / residual in either format. */
int ape_conv3x3_halo_s32_supported(const ape_conv_params* params_host);
int ape_conv3x3_halo_s32(const void* x_s32, const void* w_s32k, const float* bias, const void* residual, int res_fmt, void* y,
                         int out_fmt, const ape_conv_params* params_host, void* stream);
/* The same convolution (extractors.py:29-43; layer 4's 512 -> 512 blocks) with HALF the matrix passes: operands in the "F16M6" line format
 * (autoposeestimation_amd/mx6.py: per 32 channels fp16 values | block-scaled e2m3 codes of them | block-scaled e2m3 codes of the fp16
 * residual), x . w ~ x1 w1 + Q(x1) Q(w2) + Q(x2) Q(w1): one v_mfma_f32_16x16x32_f16 per tap and block + one
 * v_mfma_scale_f32_16x16x128_f8f6f4 per tap PAIR and block.  x from ape_s32_to_f16m6, w from mx6.pack_conv_weights; y / residual /
 * bias / activation as ape_conv3x3_halo_s32.  NOT bit-identical to the bf16x3 kernels: DESIGN.md 6e prices the difference. */
int ape_conv3x3_halo_mx_supported(const ape_conv_params* params_host);
int ape_conv3x3_halo_mx(const void* x_f16m6, const void* w_f16m6, const float* bias, const void* residual, int res_fmt, void* y,
                        int out_fmt, const ape_conv_params* params_host, void* stream);
int ape_conv3x3_halo_mx_debug(int bits);
int ape_s32_to_f16m6(const void* x_s32, void* y_f16m6, long pixels, int C, void* stream);
/* The ResNet stem in one kernel: Conv2d(3 -> 64, 7x7, stride 2, pad 3) + ReLU + MaxPool2d(3, 2, 1)  (extractors.py:82-85, 111-117).
 * x[B][H][W][4] f32 (RGB + a zero channel), w[64][7][7][4] f32 (the UNPACKED ape_conv2d_nhwc_f32 layout: the kernel splits its
 * own weight fragments), bias[64] or NULL -> y[B][Hp][Wp][64] with Ho = (H - 1) / 2 + 1, Hp = (Ho - 1) / 2 + 1 (same for W).
 * Operands as in ape_conv2d_nhwc_bf16 (nsplit 3 = split-bf16, 1 = plain bf16); the half-resolution 64-channel activation
 * between the convolution and the pool is never written. */
int ape_stem_conv_pool_bf16(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int nsplit,
                            void* stream);
/* ... and straight from the uint8 frames (pipeline/utils.py:421-427,556-560: ToTensor / Normalize of the frame or of the crop): crop o = the
 * Hc x Wc window of frame rects[o][0] at (row rects[o][1], column rects[o][2]) of rgb[n_frames][Hf][Wf][3] (rects NULL: the n = n_frames whole frames); the
 * normalisation (ape_preprocess_u8_nhwc4's arithmetic, div255 as there) runs on the way into LDS, so y is bit for bit
 * ape_stem_conv_pool_bf16(ape_preprocess_u8_nhwc4(...)) and the fp32 image is never written. */
int ape_stem_conv_pool_u8(const uint8_t* rgb, int n_frames, const int* rects, const float* w, const float* bias, float* y, int n, int Hf, int Wf,
                          int Hc, int Wc, int div255, int nsplit, void* stream);
/* 3x3 / stride 1 / pad == dilation in {1,2,4} / Cin % 32 == 0 specialisation of ape_conv2d_nhwc_bf16: the input halo of
 * a 16x16-pixel tile is staged once per 32-channel chunk in LDS and shared by the nine taps (3x less operand traffic).
 * Same arguments, packed weights, numerics and epilogue; ape_conv3x3_halo_supported(params) says whether it applies. */
int ape_conv3x3_halo_supported(const ape_conv_params* params_host);
int ape_conv3x3_halo_bf16(const float* x, const void* w_packed, const float* bias, const float* residual, float* y,
                          const ape_conv_params* params_host, int nsplit, void* stream);

/* ---- HBM-bound glue of the PSPNet / PointNet graphs (NHWC f32, C multiple of 4) -----------------------------
 * nn.MaxPool2d(3, 2, 1)                      DenseFusion/lib/extractors.py:85,117.   y[B][Ho][Wo][C], Ho=(H-1)/2+1 */
int ape_maxpool3x3s2_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, void* stream);
/* nn.AdaptiveAvgPool2d((S,S))                DenseFusion/lib/pspnet.py:15.           y[B][S][S][C] */
int ape_adaptive_avgpool_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, int S, void* stream);
/* The PSP module's pools (pspnet.py:15: sizes 2, 3, 6 of one map) in ONE pass over the map (ape_adaptive_avgpool_multi_nhwc_ld): the
 * bin edges of all sizes cut each axis into at most 12 "atoms" (APE_EINVAL otherwise: use the per-size entry point); every atom is
 * summed once into `workspace` (ape_adaptive_avgpool_multi_workspace_bytes(B, C)), then each bin adds up its atoms.  ys_host /
 * sizes_host: host arrays of nsizes <= 4 device output pointers y_i[B][S_i][S_i][C] and sizes S_i <= 8. */
size_t ape_adaptive_avgpool_multi_workspace_bytes(int B, int C);
/* F.upsample(size=(Ho,Wo), 'bilinear') / nn.Upsample(x2, align_corners=True)   pspnet.py:22,31.
 * Reads x[B][H][W][ldx] channels 0..C-1, writes y[B][Ho][Wo][ldy] channels yoff..yoff+C-1 (a slice of the PSP
 * concat buffer, pspnet.py:22-23); accumulate != 0 adds into y instead of overwriting. */
int ape_bilinear_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, int ldx, int Ho, int Wo, int ldy,
                          int yoff, int align_corners, int accumulate, void* stream);
/* sum over the four PSP priors of F.upsample(prior_s, size=(h,w), 'bilinear') (pspnet.py:22, align_corners=False), z_s[B][s][s][C]
 * for s = 1,2,3,6 -> out[B][h][w][C]; one pass instead of four accumulating ape_bilinear_nhwc_f32 passes, same summation order */
int ape_psp_prior_sum_f32(const float* z1, const float* z2, const float* z3, const float* z6, float* out, int B, int h,
                          int w, int C, void* stream);
/* PSPUpsample (nn.Upsample x2 align_corners=True -> Conv2d 3x3 pad 1 -> PReLU, pspnet.py:27-37) restructured: the 3x3 conv's
 * channel mixing runs at LOW resolution as a 1x1 conv producing z[B][h][w][9*C] (channel = tap*C + c, tap = ky*3+kx, made by
 * ape_conv2d_* from the repacked weights W'[(tap,co)][ci]); this kernel resizes, shifts by the tap, sums, adds bias and
 * applies the activation: out[B][2h][2w][C].  Exact up to fp32 rounding (conv and bilinear resize are both linear). */
int ape_upconv3x3_gather_f32(const float* z, const float* bias, float* out, int B, int h, int w, int C, int act, float alpha,
                             void* stream);
/* torch.gather(emb, 2, choose)               DenseFusion/lib/network.py:100-102.     y[b][i][:] = x[b][index[b][i]][:] */
int ape_gather_rows_f32(const float* x, const int64_t* index, float* y, int B, int rows_in, int n, int C, void* stream);
/* 3x3 patches of nn.Upsample(x2, align_corners=True)(x) at chosen pixels only: x[B][h][w][C] (C % 4 == 0), index[B][n] i64 = pixel
 * y * 2w + x of the up-sampled image -> out[B*n][9*C], column = (ky*3+kx)*C + c, zero where the tap falls outside the 2h x 2w
 * image.  With the up_3 weights read as a [Cout][9*C] matrix (their packed layout already is one) a single 1x1 contraction
 * then evaluates pspnet.py:30-33 at the N points network.py:100-102 keeps, instead of at all Hc*Wc pixels of the crop. */
int ape_ups_patch_gather_f32(const float* x, const int64_t* index, float* out, int B, int h, int w, int C, int n, void* stream);
/* nn.LogSoftmax() over the channel run       DenseFusion/lib/pspnet.py:55.           rows x C, C contiguous */
int ape_log_softmax_rows_f32(const float* x, float* y, long rows, int C, void* stream);
/* nn.AvgPool1d(num_points)                   DenseFusion/lib/network.py:51,65,149,166.  x[B][n][C] -> y[B][C] */
int ape_mean_rows_f32(const float* x, float* y, int B, int n, int C, void* stream);
/* x[rows][3] -> y[rows][4] (w = 0): lets the first 1x1 conv (network.py:42,139) use 16-byte loads */
int ape_pad3to4_f32(const float* x, float* y, long rows, void* stream);
/* conv4_r / conv4_t / conv4_c + sigmoid + index_select(obj)   DenseFusion/lib/network.py:115-126 (and the refiner's
 * conv3_r / conv3_t, :197-204, with wc = bc = NULL): only the selected object's 8 output rows are evaluated.
 * h[B*n][ldh] holds the K-wide inputs of the three heads at channel offsets off_r/off_t/off_c; obj[B] i64;
 * out[B][n][8] = (qw,qx,qy,qz, tx,ty,tz, sigmoid(c)). */
int ape_head_select_f32(const float* h, int ldh, int off_r, int off_t, int off_c, const float* wr, const float* br,
                        const float* wt, const float* bt, const float* wc, const float* bc, const int64_t* obj,
                        float* out, int B, int n, int K, void* stream);

/* ---- pose extraction / composition, device resident ----------------------------------------------------------
 * my_estimator_prediction + get_new_points   DenseFusion/tools/utils.py:7-18,43-86.
 * heads[B][n][8] (from ape_head_select_f32), points4[B][n][4] -> pose[B][7] f64 (qw,qx,qy,qz,tx,ty,tz),
 * which[B] (arg-max confidence, may be NULL), new_points4[B][n][4] (may be NULL). */
int ape_pose_select_f32(const float* heads, const float* points4, double* pose, int* which, float* new_points4,
                        int B, int n, void* stream);
/* The two above for a caller that wants the pose only (my_estimator_prediction reads r and t at ONE row per crop): the confidence head on
 * every row, the r / t heads on the selected row.  Same arithmetic and the same first-maximum rule as ape_head_select_f32 followed by
 * ape_pose_select_f32, bit for bit.
 * ape_head_conf_argmax_f32: h3c[B*n][ldh] holds the K-wide input of the confidence head at channel offset off_c (16-byte aligned base,
 * ldh, off_c and K multiples of 4, K <= 1024) -> which[B] (arg-max of sigmoid(c) over the crop's n rows), conf[B] (that value), and, when
 * pf != NULL, pf_row_out[B][ld_pf] = pf[b*n + which[b]][0..ld_pf).
 * ape_pose_from_row_f32: h3rt_row[B][ldh] holds the K-wide inputs of the r and t heads of each crop's selected row at off_r / off_t;
 * which[B] as written above -> pose[B][7] f64 and new_points4[B][n][4] (may be NULL) as ape_pose_select_f32 writes them. */
int ape_head_conf_argmax_f32(const float* h3c, int ldh, int off_c, const float* wc, const float* bc, const int64_t* obj,
                             int* which_out, float* conf_out, const float* pf, int ld_pf, float* pf_row_out, int B, int n, int K,
                             void* stream);
int ape_pose_from_row_f32(const float* h3rt_row, int ldh, int off_r, int off_t, const float* wr, const float* br, const float* wt,
                          const float* bt, const int64_t* obj, const int* which, const float* points4, double* pose,
                          float* new_points4, int B, int n, int K, void* stream);
/* my_refined_prediction                     DenseFusion/tools/utils.py:20-40 (+ transformations.py:1254-1278,1320-1363).
 * pose[B][7] f64 is updated in place with the refiner residual ref_r[B][ldr>=4], ref_t[B][ldt>=3] (f32). */
int ape_pose_compose_f64(double* pose, const float* ref_r, int ldr, const float* ref_t, int ldt, int B, void* stream);
/* cloud re-centring of the iterative loop    DenseFusion/tools/eval_ycb.py:205-210. */
int ape_pose_recentre_f32(const float* points4, const double* pose, float* new_points4, int B, int n, void* stream);

/* ---- ADD / ADD-S and the DenseFusion loss forward -------------------------------------------------------------
 * loss_calculation               DenseFusion/lib/loss.py:12-73, lib/loss_refiner.py:12-64, tools/eval_linemod.py:118-130.
 * pred[n][m] = R(pred_r[n]/|pred_r[n]|) . model[m] + pred_t[n] (+ points[n] when points != NULL, loss.py:38);
 * dis[n] = mean_m |pred[n][m] - target[m']|, m' = m, or for symmetric objects the nearest target with the k-NN
 * kernel's float32 arithmetic and lowest-index tie rule (loss.py:42-47); stdv[n] = unbiased std of those norms (may be
 * NULL); pred_out[N][M][3] is written only when non-NULL.  pred_r[N][4], pred_t[N][3], points[N][3], model/target[M][3]. */
int ape_adds_dis_f32(const float* pred_r, const float* pred_t, const float* points, const float* model,
                     const float* target, int N, int M, int symmetric, float* pred_out, float* dis, float* stdv,
                     void* stream);
/* The evaluation form (DenseFusion/tools/eval_linemod.py:118-130, experiments/eval.py:75-95) for a BATCH of objects in one launch: pose b
 * (pred_r[b] unnormalised wxyz, pred_t[b]) places ITS model cloud model[b][M][3] and is scored against ITS target[b][M][3]; symmetric:
 * every predicted point against its nearest target (the k-NN kernel's arithmetic and tie rule, several lanes per point like ape_knn_f32).
 * dis[b] = ADD / ADD-S in the clouds' unit, bit for bit ape_adds_dis_f32's value for that object alone. */
int ape_adds_dis_batched_f32(const float* pred_r, const float* pred_t, const float* model, const float* target, int B, int M, int symmetric,
                             float* workspace /* B * M floats */, float* dis, void* stream);
/* loss = mean((dis + 2 std) c - w log c), which = argmax c (first), out9 = (loss, dis[which], pred_r[which][0..3],
 * pred_t[which] + points[which])   loss.py:50-59 */
int ape_adds_select_f32(const float* dis, const float* stdv, const float* pred_c, const float* pred_r,
                        const float* pred_t, const float* points, int N, float w, float* out9, int* which,
                        void* stream);
/* out[i] = (pts[i] - t) . ori_base(q/|q|), qt7 = (q[4], t[3]) on the device   loss.py:61-69, loss_refiner.py:51-60 */
int ape_recentre_qt_f32(const float* pts, const float* qt7, float* out, int n, void* stream);
/* The YCB-Video toolbox's four pose errors    DenseFusion/replace_ycb_toolbox/evaluate_poses_keyframe.m:148-217 (csrc/pose_errors.hip)
 * for n_inst ground-truth objects x n_src pose sources in one call, float64 throughout.  models[n_points][3]: the model points of all
 * classes; offsets[n_models + 1] i32: class c owns rows offsets[c] .. offsets[c + 1] (no upper limit on a model's length; m_max: the
 * longest one, which sizes the workspace); cls[n_inst] i32 0-based; rt_gt[n_inst][12], rt_est[n_inst][n_src][12]: row-major 3 x 4;
 * valid[n_inst][n_src] u8.  out[n_inst][n_src][4] = (adi, add, re, te):
 *   adi  mean_i min_j |(R_gt p_i + t_gt) - (R_est p_j + t_est)|  (exhaustive search, squared distance (dx dx + dy dy) + dz dz, no FMA)
 *   add  mean_i |(R_est p_i + t_est) - (R_gt p_i + t_gt)|
 *   re   180 / pi acos(clamp(0.5 (trace(R_est inv(R_gt)) - 1), -1, 1)) with the general 3 x 3 inverse; te  |t_gt - t_est|
 * valid == 0: four +inf, the pose is not read.  A class outside the table, or a model the table places outside models / makes longer than
 * m_max: four NaN, nothing else is read.  est == gt gives four exact zeros.  Sums run in one fixed order, the same for every number of
 * lanes per query the call may choose: results are bit-identical from run to run and from call size to call size.  All pointers are device memory. */
int ape_pose_errors_chunk(void);      /* reference points per LDS chunk */
int ape_pose_errors_queries(void);    /* model points a workgroup owns at one lane per point (fewer by the factor below otherwise) */
int ape_pose_errors_lanes(long n_pairs, int m_max);   /* 1, 4, 16 or 64 lanes per model point for a call of n_pairs = n_inst * n_src */
size_t ape_pose_errors_workspace_bytes(long n_pairs, int m_max);
int ape_pose_errors_f64(const double* models, const int* offsets, int n_models, long n_points, const int* cls, const double* rt_gt,
                        const double* rt_est, const unsigned char* valid, long n_inst, int n_src, int m_max, double* out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- segmentation post-processing, crop / point selection (byte and index work, bit-exact) ----------------------
 * softmax(+softmax) / argmax                 pipeline/utils.py:429-435 (predict's softmax activation, create_labels.py:23,
 * then F.softmax again, then torch.argmax).  logits[npix][ld] f32 (first C channels) -> label[npix] u8,
 * score[npix] f32 = probability of the arg-max class after one (double_softmax=0) or two softmaxes. */
int ape_seg_argmax_f32(const float* logits, int ld, int C, uint8_t* label, float* score, long npix,
                       int double_softmax, void* stream);
/* Fused segmentation head: the 64 -> C final 1x1 conv (pspnet.py:53-55, first C rows) + softmax(+softmax) + argmax in one
 * pass over feat[npix][64] f32, without the logits tensor.  C <= 16.  Against ape_conv2d_* followed by ape_seg_argmax_f32: the head
 * sums the 64 channels on the matrix cores (another fp32 order) and takes its exponentials / its reciprocal from v_exp_f32 / v_rcp_f32
 * (1 ulp) where ape_seg_argmax_f32 uses expf and IEEE divisions, so scores agree to ~1e-6 and labels agree except where two classes'
 * final float32 probabilities are within 1 ulp of each other (the tie band torch.argmax resolves to the lowest index; for a top
 * probability below 0.5 one ulp of p decides exp(p - pmax) == 1).  Every fused form of this head in the library (this entry,
 * ape_conv3x3_halo_seghead_bf16, ape_upconv3x3_fused_seghead_s32) runs the SAME code (csrc/seg_head.h) and they agree bit for bit;
 * tests/test_gpu_segpost.py and bench.py's parity block count label differences outside the band only. */
int ape_seg_head_f32(const float* feat, const float* w, const float* bias, int C, uint8_t* label, float* score, long npix,
                     int double_softmax, void* stream);
/* np.unique counts + cv2.connectedComponents(8) + best mean-probability component + mask + get_bbox
 *   pipeline/utils.py:437-469, DenseFusion/datasets/myDatasetAugmented/dataset.py:338-380.
 * label/score[B][H][W] -> objmap[B][H][W] u8 (class id inside the winning component of that class, else 0; the
 * reference's per-class mask is (objmap == cls) * 255) and det[B][C][5] i32 = (valid, rmin, rmax, cmin, cmax).
 * Classes with <= min_pixels pixels are skipped (reference: 100); the count is the class's in the frame, not one component's.
 * label may hold ANY byte: a label of 0 or >= C takes part in nothing -- it is not counted, belongs to no component, scores for no
 * class, objmap is 0 there and no det row depends on it (the result equals the run with those pixels set to 0).  1 <= C <= 64,
 * B H W < 2^31 - 1, B < 65536 (the frame is a grid y index). */
size_t ape_seg_components_workspace_bytes(int B, int H, int W, int C);
/* The component score is selectable: APE_SEG_SCORE_MEAN = mean probability (pipeline/utils.py:456-462),
 * APE_SEG_SCORE_SUM = summed probability, the rule of do_cca (background_subtraction/utils.py:199-222: label 0/1,
 * biggest = arg max_u sum(max-prob[labels == u]), first component wins ties). */
#define APE_SEG_SCORE_MEAN 0
#define APE_SEG_SCORE_SUM 1
int ape_seg_components_scored(const uint8_t* label, const float* score, uint8_t* objmap, int* det, int B, int H, int W,
                              int C, int min_pixels, int score_mode, void* workspace, size_t workspace_bytes, void* stream);
/* Background-subtraction network input   background_subtraction/utils.py:721-828 (get_mask_prediction's per-frame block):
 * f_rgb/b_rgb[B][H][W][3] u8 and f_depth/b_depth[B][H][W] u16 of the object frame and of the empty-scene frame taken from
 * the same view point -> the 7 channels |dRGB|, |dHSV| (Pillow's 8-bit HSV), |d depth| (gate [min,max] per frame, :747-763,
 * gate_min_max[B][2] f64 on the DEVICE), each cast to uint8 as numpy does (:811, the depth channel wraps mod 256), then
 * ToTensor + Normalize(mean7, std7) (:818-819; HOST pointers).  out[B][H][W][8] f32 NHWC (channel 7 = 0);
 * diff_or_null[B][H][W][7] receives the uint8 channels when not NULL. */
int ape_bgsub_features_f32(const uint8_t* f_rgb, const uint8_t* b_rgb, const uint16_t* f_depth, const uint16_t* b_depth,
                           const double* gate_min_max, const float* mean7_host, const float* std7_host, float* out,
                           uint8_t* diff_or_null, int B, int H, int W, void* stream);
/* trust checks of the relabelling loop   label_generator/create_labels.py:166-196.  objmap from ape_seg_components_scored
 * (min_pixels = 0), cls = target class; counts[B][6] u32 (zeroed by the caller) = (bs&pred, bs&!pred, depth&pred,
 * depth&!pred, centre&pred, centre&!pred) with the depth gate [min,max] per frame (:106-112) and the 30/50 px centre window. */
int ape_label_trust_counts(const uint8_t* objmap, int cls, const uint8_t* bs_label_or_null, const uint16_t* depth,
                           const float* gate_min_max, int B, int H, int W, int cut0, int cut1, unsigned int* counts,
                           void* stream);
/* choose = mask[rmin:rmax, cmin:cmax].flatten().nonzero(); > N -> ordered subset, <= N -> wrap pad
 *   pipeline/utils.py:524-539.  objects[n][6] i32 = (frame, cls, rmin, rmax, cmin, cmax);
 * choose[n][N] i64 indices inside the crop; n_cand[n] (0 => object dropped, :530-531); cand: scratch [n][cand_stride]. */
int ape_choose_points(const uint8_t* objmap, const uint16_t* depth, const int* objects, int n, int H, int W, int N,
                      unsigned int seed, int* cand, long cand_stride, int64_t* choose, int* n_cand, void* stream);
/* the same with the sampling seed read from DEVICE memory when the kernel runs: a launch captured in a HIP graph then follows a seed that
 * the host updates between replays (pipeline/utils.py FramePipeline(pose_graphs=True)) */
int ape_choose_points_dseed(const uint8_t* objmap, const uint16_t* depth, const int* objects, int n, int H, int W, int N,
                            const unsigned int* seed_device, int* cand, long cand_stride, int64_t* choose, int* n_cand, void* stream);
/* float32 pin-hole back-projection          pipeline/utils.py:542-553.  points4[n][N][4] = (x, y, z, 0) */
int ape_backproject_f32(const uint16_t* depth, const int* objects, const int64_t* choose, float* points4, int n,
                        int H, int W, int N, float fx, float fy, float ppx, float ppy, float depth_scale, void* stream);
/* ToTensor(/255)+Normalize (pipeline/utils.py:421-427, div255=1) or raw-scale crop normalisation (:559-560, div255=0):
 * rgb[B][H][W][3] u8, rects[n][3] i32 = (frame, row0, col0) -> out[n][Hc][Wc][4] f32 (channel 3 = 0). */
int ape_preprocess_u8_nhwc4(const uint8_t* rgb, const int* rects, float* out, int n, int H, int W, int Hc, int Wc,
                            int div255, void* stream);

/* ---- pose-label path: point clouds in float64 (pc_reconstruction/open3d_utils.py, open3d 0.9 semantics) -------
 * The path's primitives are the `*_batch_f64` calls further down (a cloud alone is a batch of one); here: the all-pairs k-NN that the
 * grid search is tested against, and the two steps of one ICP evaluation as calls of their own for a loop that solves on the host (the
 * LAPACK check of the device step): one-record calls of the kernels of ape_icp_run_batch_f64 over ONE cloud's grid. */
/* registration_icp's correspondence search: nearest target point within max_dist, idx = -1 if none   :98-117 */
int ape_grid_nn1_f64(const double* sorted, const unsigned long long* keys, const unsigned* order, const double* origin3,
                     int n, double cell, const double* q, int nq, double max_dist, int* idx, double* dist2, void* stream);
/* remove_statistical_outlier's per-point mean distance to its k nearest neighbours (self included)   :208-211 */
int ape_knn_mean_dist_f64(const double* pts, int n, int k, double* mean, void* stream);
/* One-pass ICP reductions (bitwise reproducible).  kind 0: point-to-point (Umeyama) out[17] = count, sum d^2, sum s[3],
 * sum t[3], sum s_a t_b[9];  kind 1: point-to-plane out[29] = count, sum d^2, upper triangle of J^T J[21], J^T r[6];
 * kind 2: moments of src, out[9] = sum p[3], sum p_a p_b upper triangle[6] (get_center / compute_mahalanobis_distance).
 * ws: 512 x 29 doubles. */
int ape_icp_sums_f64(int kind, const double* src, const double* tgt, const double* tgt_normals, const int* corr,
                     const double* dist2, int n, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- the point-cloud primitives, BATCHED (pose-label path, SURVEY.md 8e: the (object, direction) chains of
 * pc_reconstruction/create_pointcloud.py:276-312 are independent of each other).  ONE launch advances up to 16 clouds: blockIdx.y selects
 * the cloud's argument record, blockIdx.x walks that cloud's own grid, whose size depends on that cloud's point count alone -- a cloud's
 * result does not depend on its slot or its neighbours in the batch.  Per-cloud arguments are HOST arrays (of device pointers / sizes) of
 * length nb <= 16; clouds with n = 0 are skipped.  hipCUB's radix sort becomes a single-workgroup LDS sort per cloud (the cell keys re-coded
 * as a 32-bit lexicographic rank, packed with the index: stable, the same permutation), its select / scan calls a single-workgroup ordered
 * compaction / scan per cloud. */
size_t ape_pc_batch_workspace_bytes(int nb, long n_total);
/* get_surface's pixel loop        pc_reconstruction/open3d_utils.py:171-192: pixels with label != 0 and depth != 0, in raster
 * order, back-projected (mm, no depth scale) and moved to the robot frame by T (row-major 4x4).
 * label[c] / depth[c] [H][W]; intr4_host [nb][4] = fx, fy, ppx, ppy; T16_host [nb][16]; points[c] capacity H*W rows;
 * n_out [nb] on the device; pix_ws: nb * H * W ints of scratch */
int ape_surface_points_batch_f64(int nb, const uint8_t* const* label, const uint16_t* const* depth, int H, int W, const double* intr4_host,
                                 const double* T16_host, double* const* points, int* n_out, int* pix_ws, void* stream);
/* PointCloud.voxel_down_sample    open3d_utils.py:21,198,157: per-voxel mean, output ordered by voxel key; out[c] capacity n[c] rows */
int ape_voxel_down_sample_batch_f64(int nb, const double* const* pts, const int* n, double voxel, double* const* out, int* n_out, void* ws,
                                    size_t ws_bytes, void* stream);
/* Uniform search grid over a cloud (cell >= every radius later asked of it): caller-owned sorted[c][n][3], keys[c][n],
 * order[c][n], origin3[c][3].  Replaces open3d's KDTreeFlann for the bounded-radius searches of the path. */
int ape_grid_build_batch_f64(int nb, const double* const* pts, const int* n, double cell, double* const* sorted, unsigned long long* const* keys,
                             unsigned* const* order, double* const* origin3, void* ws, size_t ws_bytes, void* stream);
/* op 0: remove_radius_outlier's neighbour count (d < radius, self included; open3d_utils.py:203) -> count[c][nq[c]];
 * op 1: estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) (:25-27), normals oriented towards +z -> normals[c][nq[c]][3];
 * op 2: the means of ape_knn_mean_dist_f64 for the grid's own points, searched shell by shell through the grid instead of over all
 *       pairs: bitwise equal for any cell size; fastest when a cell holds a few points (cell ~ the radius that contains k neighbours).
 *       k <= 64, k <= gn[c] -> mean[c][gn[c]]; q / nq unused */
int ape_grid_query_batch_f64(int op, int nb, const double* const* sorted, const unsigned long long* const* keys, const unsigned* const* order,
                             const double* const* origin3, const int* gn, double cell, const double* const* q, const int* nq, double radius,
                             int max_nn_or_k, int* const* count, double* const* normals, double* const* mean, void* stream);
/* ordered row selection (outlier filters) with the keep rule evaluated on the device: mode 0 count[c][i] > thr_count
 * (RemoveRadiusOutliers), mode 1 mean[c][i] > 0 && mean[c][i] < thr_mean_host[c] (RemoveStatisticalOutliers).  out[c] = the kept rows
 * (capacity n[c]), n_out [nb] on the device; sel_ws: sum n ints, cloud c's kept indices at offset n[0] + .. + n[c-1] */
int ape_select_points_batch_f64(int mode, int nb, const double* const* pts, const int* n, const int* const* count, int thr_count,
                                const double* const* mean, const double* thr_mean_host, double* const* out, int* n_out, int* sel_ws, void* stream);
/* the moments of ape_icp_sums_f64(kind 2): out9 [nb][9] on the device; ws: nb * 512 * 9 doubles */
int ape_moments_batch_f64(int nb, const double* const* pts, const int* n, double* out9, void* ws, size_t ws_bytes, void* stream);
/* compute_mahalanobis_distance    mc12_host [nb][12] = (mean[3], inverse covariance[9]) */
int ape_mahalanobis_batch_f64(int nb, const double* const* pts, const int* n, const double* mc12_host, double* const* out, void* stream);
/* PointCloud.transform            in place, T16_host [nb][16]; normals (may be NULL, per cloud too) get the rotation part */
int ape_transform_points_batch_f64(int nb, double* const* pts, double* const* normals, const int* n, const double* T16_host, void* stream);
/* out[c] = [a[c] | b[c]] (b may be NULL: copies) */
int ape_concat_points_batch_f64(int nb, const double* const* a, const int* na, const double* const* b, const int* nb_rows, double* const* out,
                                void* stream);
/* registration_icp's LOOP on the device (open3d_utils.py:96-117; open3d 0.9 RegistrationICP) for nb registrations of one kind advancing
 * together: `n_iter` iterations of [move src by the pending update + correspondence search] -> partial sums -> [reduce + step: fitness /
 * rmse / convergence test, Umeyama 3x3 SVD (kind 0) or 6x6 solve (kind 1), T <- update . T], three launches each, enqueued at once; for a
 * registration every launch is a no-op once its state[0] != 0.  first_call = 1 prepends the evaluation before open3d's loop and the step
 * that computes the first update.  `src[c]` is the source already moved by the initial guess, updated in place.  state[c]: 40 doubles on
 * the device: [0] done, [1] updates applied, [2] fitness, [3] inlier rmse, [4] correspondences, [5..20] T row major, [21..36] last
 * update, [37] stop reason (1 converged, 2 too few correspondences, 3 iteration limit), [38] internal.  Before the first call of a
 * registration (first_call = 1) the caller zeroes it and writes the initial T; one copy of it back per call tells whether to enqueue
 * more.  Grid arguments: the targets' grids (cell >= max_dist); ws: nb * 512 * 29 doubles.  sums[c][29], corr[c][ns], dist2[c][ns]:
 * caller-owned scratch. */
int ape_icp_run_batch_f64(int kind, int nb, const double* const* sorted, const unsigned long long* const* keys, const unsigned* const* order,
                          const double* const* origin3, const int* gn, double cell, double* const* src, const int* ns, const double* const* tgt,
                          const double* const* tgt_normals, double max_dist, double rel_fitness, double rel_rmse, int max_iteration, int n_iter,
                          int first_call, int* const* corr, double* const* dist2, double* const* sums, double* const* state, void* ws,
                          size_t ws_bytes, void* stream);

/* ---- global registration (reference pc_reconstruction/open3d_utils.py:19-49; open3d 0.9 compute_fpfh_feature and
 * registration_ransac_based_on_feature_matching), float64, autoposeestimation_amd/csrc/registration.hip ----------------------------
 * Every call takes nb = 1..16 clouds / pairs per launch (APE_EINVAL otherwise); a single cloud or pair is a call with nb = 1, there are no
 * one-pair entry points.  The kernels take a by-value table of per-pair records and the pair's index in a grid dimension.  Per-pair
 * arguments are HOST arrays [nb] of device pointers / sizes (as the `*_batch_f64` point-cloud calls); a pair's result depends on that
 * pair alone, not on its slot or its neighbours.  Workspaces: the pairs' own regions one after the other.
 * FPFH feature[c][n][33] of nb clouds with normals (pts[c] / normals[c] [n][3] in the cloud's own order) through their search grids (the
 * buffers of ape_grid_build_batch_f64 over the same points, gn[c] points, cell >= radius): hybrid neighbour list d^2 < radius^2, ordered by
 * (d^2, index), first max_nn (<= 128); SPFH over the list without its entry 0, then FPFH = per 11-bin block normalised
 * sum_k SPFH_k / d^2_k (d^2 != 0) + SPFH_i.  Points with at most one list entry get zeros.  Two launches; a cloud with gn[c] == 0 is
 * skipped.  Workspace: for n_host[nb] points per cloud and the given max_nn. */
size_t ape_fpfh_batch_workspace_bytes(int nb, const int* n_host, int max_nn);
int ape_fpfh_batch_f64(int nb, const double* const* sorted, const unsigned long long* const* keys, const unsigned* const* order,
                       const double* const* origin3, const int* gn, double cell, const double* const* pts, const double* const* normals,
                       double radius, int max_nn, double* const* feature, void* ws, size_t ws_bytes, void* stream);
/* Nearest target feature for nb (source, target) feature pairs in two launches: nn[c][s] = argmin_t sum_j (src_feature[c][s][j] -
 * tgt_feature[c][t][j])^2 over the 33 dimensions in j order, fp64, ties -> lowest t.  A pair with ns[c] == 0 or nt[c] == 0 is skipped (its
 * nn is not written).  The target range of a pair is cut into slices so that the whole launch has about 2048 blocks. */
size_t ape_feature_nn1_batch_workspace_bytes(int nb, const int* ns_host, const int* nt_host);
int ape_feature_nn1_batch_f64(int nb, const double* const* src_feature, const int* ns, const double* const* tgt_feature, const int* nt,
                              int* const* nn, void* ws, size_t ws_bytes, void* stream);
/* Workspace of the two RANSAC calls below (ns_host[nb] source sizes): hypotheses in chunks of up to `chunk` iterations, up to
 * max_validation kept per pair. */
size_t ape_ransac_batch_workspace_bytes(int nb, const int* ns_host, int chunk, int max_validation);
/* RANSAC iterations [it_begin, it_begin + n_it) for every pair whose list is not yet full: iteration i of pair c draws source
 * s_j = splitmix64(((uint64_t)seed_host[c] << 32) ^ (i * ransac_n + j)) mod ns[c], j < ransac_n (3..16), pairs it with nn[c][s_j], runs the
 * edge-length checker (edge_sim < 0: none), Umeyama without scaling and the distance checker (dist_thr < 0: none).  The passing
 * iteration indices are appended IN ITERATION ORDER to kept[c * max_validation ..] / n_kept[c] (device, n_kept zeroed by the caller
 * before the first chunk) until max_validation are kept; a pair whose n_kept[c] has reached max_validation turns its blocks into no-ops
 * by reading that word.  ns[c], nt[c] >= 1.  Two launches. */
int ape_ransac_hypotheses_batch_f64(int nb, const double* const* src, const int* ns, const double* const* tgt, const int* nt,
                                    const int* const* nn, int ransac_n, const long* seed_host, double edge_sim, double dist_thr,
                                    int it_begin, int n_it, int max_validation, int* kept, int* n_kept, void* ws, size_t ws_bytes,
                                    void* stream);
/* Models, validation and selection of all pairs in three launches: pair c validates the n_kept_host[c] (host count, <= 65535 and
 * <= kept_stride) iterations kept[c * kept_stride ..] (kept non-NULL, kept_stride >= 1 even when every count is 0): each one's
 * transformation recomputed, every source point moved by it and matched to its nearest target within max_dist (d^2 < max_dist^2; the
 * grid arguments are the targets', cell >= max_dist, gn[c] == nt[c]); fitness = count / ns, rmse = sqrt(sum d^2 / count) (0 without
 * matches), fixed-order sums.  result[nb][24] on the device, per pair: [0..15] the winner's 4x4 (row major), [16] fitness, [17] rmse,
 * [18] correspondences, [19] its position in kept, [20] its iteration (-1 / -1 and the identity with fitness 0 when nothing is better
 * than that); the winner has the highest fitness, then the lowest rmse, then the lowest iteration.  fit_rmse: NULL or [nb] pointers
 * (NULL or [n_kept_host[c]][3] on the device: fitness, rmse, correspondences of every kept iteration). */
int ape_ransac_validate_batch_f64(int nb, const double* const* sorted, const unsigned long long* const* keys, const unsigned* const* order,
                                  const double* const* origin3, const int* gn, double cell, const double* const* src, const int* ns,
                                  const double* const* tgt, const int* nt, const int* const* nn, int ransac_n, const long* seed_host,
                                  const int* kept, int kept_stride, const int* n_kept_host, double max_dist, double* result,
                                  double* const* fit_rmse, void* ws, size_t ws_bytes, void* stream);

/* ---- fast global registration (Zhou, Park, Koltun 2016; open3d 0.9 registration_fast_based_on_feature_matching restated, DESIGN.md
 * section 6g) for nb <= 16 pairs in lock step; a pair with ns[c] == 0 or nt[c] == 0 is skipped (its pointers may be NULL).
 * Mutual matches: the pairs (i, nn_st[c][i]) with nn_ts[c][nn_st[c][i]] == i, in ascending i, to mutual_s[c] / mutual_t[c] (capacity
 * min(ns[c], nt[c]) ints each) and their count to n_mutual[c] (device, [nb]).  One launch. */
int ape_fgr_mutual_batch(int nb, const int* const* nn_st, const int* ns, const int* const* nn_ts, const int* nt, int* const* mutual_s,
                         int* const* mutual_t, int* n_mutual, void* stream);
/* Workspace of ape_fgr_tuples_batch_f64 for chunks of up to `chunk` trials. */
size_t ape_fgr_workspace_bytes(int nb, int chunk);
/* The tuple test, trials [trial_begin, trial_begin + n_trials) below the pair's own limit of 100 * n_mutual[c]: trial t draws the three
 * positions r_k = splitmix64(((uint64_t)seed << 32) ^ (3 t + k)) mod n_mutual[c] of the mutual list and passes when, for each of the edges
 * 0-1, 1-2 and 2-0, the source length li and the target length lj satisfy li * tuple_scale < lj and lj * tuple_scale < li.  The passing
 * trial indices are appended IN TRIAL ORDER to kept[c * max_tuples ..] / n_kept[c] (device; the caller zeroes n_kept before the first
 * chunk) until max_tuples are kept; a full pair's blocks are no-ops.  Two launches. */
int ape_fgr_tuples_batch_f64(int nb, const double* const* src, const int* ns, const double* const* tgt, const int* nt,
                             const int* const* mutual_s, const int* const* mutual_t, const int* n_mutual, const long* seed_host,
                             double tuple_scale, int trial_begin, int n_trials, int max_tuples, int* kept, int* n_kept, void* ws,
                             size_t ws_bytes, void* stream);
/* Centring / scale and the optimisation, two launches.  norm8[nb][8] (device, written): mean and largest centred norm of the source,
 * then of the target.  Pair c's correspondences are the three re-drawn pairs of each of its n_kept_host[c] <= 1000 kept trials
 * (kept[c * kept_stride ..]); fewer than 10 give the identity.  One workgroup per pair holds them in LDS, runs iteration_number
 * Gauss-Newton steps (27 fixed-order sums, 6x6 LDL^T, T <- update . T) and stops early at a pivot that is not finite and positive.
 * result[nb][24] (device): [0..15] T in the clouds' units, [16] iterations run, [17] scale, [18] the last par, [19] correspondences. */
int ape_fgr_optimize_batch_f64(int nb, const double* const* src, const int* ns, const double* const* tgt, const int* nt,
                               const int* const* mutual_s, const int* const* mutual_t, const int* n_mutual, const long* seed_host,
                               const int* kept, int kept_stride, const int* n_kept_host, int use_absolute_scale, int decrease_mu,
                               double division_factor, double max_corr_dist, int iteration_number, double* norm8, double* result,
                               void* stream);

/* ---- depth ICP polish of the pose stage (csrc/icp_polish.hip) ------------------------------------------------------------------------
 * For each of n objects: open3d 0.9 RegistrationICP with TransformationEstimationPointToPoint (the loop of ape_icp_run_batch_f64,
 * kind 0) of the object's observed points onto its class's model cloud, all iterations in ONE launch, one workgroup per object; nothing
 * is read back or allocated, and no argument is a host array, so the call can be captured in a HIP graph.
 *   points4[n][N][4] f32   what ape_backproject_f32 wrote (camera frame, metres); object i's source is its first
 *                          ns = min(n_cand[i], N) rows widened to float64 -- the rows behind them are never read.  N <= 2048.
 *   obj_class[n] i32       row of model_table the object registers to
 *   model_table[n_classes][5] i64 (device, built once per cloud set): the addresses of the class's search grid as
 *                          ape_grid_build_batch_f64 wrote it -- sorted [M][3] f64, keys [M] u64, order [M] u32, origin [3] f64 -- and M.
 *                          Every grid has cell size `cell` >= max_dist; max_model_points >= every M (it sizes the LDS staging of the
 *                          grid: a class with more points is searched in global memory).
 *   pose_in[n][7] f64      (w, x, y, z, tx, ty, tz) as the pose stage leaves it; init = inverse([R(q / |q|) | t])
 *   pose_out[n][7] f64     inverse(T), quaternion as ape_pose_compose_f64 writes it (q[0] >= 0)
 *   stats[n][4] f64        fitness, inlier rmse, correspondences, stop reason (1 converged by the relative criteria, 2 fewer than 3
 *                          correspondences, 3 iteration limit: state[37] of ape_icp_run_batch_f64)
 * pose_out[i] is pose_in[i] bit for bit when no update was applied (ns < 3, too few correspondences at the first evaluation,
 * max_iteration 0) and when the final fitness is below min_fitness (stats stay the registration's).  An object with ns == 0 reports
 * (0, 0, 0, 2), and so does one whose table row has M < 1.  obj_class lives on the device, so a class outside the table cannot be
 * refused on the host: such an object passes its pose through with stats (0, 0, 0, 0).  The sums are added in an order that depends
 * on ns alone: an object's result has the same bits alone and in any batch.
 * APE_EINVAL (with ape_last_error): n < 0, N outside 1..2048, max_dist <= 0, cell < max_dist, an empty table, max_iteration < 0. */
int ape_icp_polish_batch_f64(int n, const float* points4, const int* n_cand, int N, const int* obj_class, const int64_t* model_table,
                             int n_classes, int max_model_points, double cell, const double* pose_in, double max_dist,
                             double relative_fitness, double relative_rmse, int max_iteration, double min_fitness, double* pose_out,
                             double* stats, void* stream);

/* ape_icp_polish_batch_f64 with TransformationEstimationPointToPlane (the loop of ape_icp_run_batch_f64, kind 1) on the model clouds'
 * normals; the same launch shape, buffers, pass-through rules and refusals, and:
 *   normals_table[n_classes] i64 (device, built once per cloud set): the address of the class's normals, [M][3] f64 in the order of
 *                          the cloud's points (row order[j] belongs to sorted[j]); neither sign nor length matters to the fixed
 *                          point's existence -- J and r flip together -- but the normals are used as given.  They are read from
 *                          global memory whether or not the grid is staged into LDS.
 *   stats[n][4] f64        stop reason 2 is "fewer than 6 correspondences"
 * An update is the solution x of (J^T J) x = -J^T r over the correspondences, r = (s - t).n_t, J = [s x n_t, n_t], applied as
 * Rz(x2) Ry(x1) Rx(x0) with translation x[3..5]; an exactly singular system gives the identity update, which counts as an update (so
 * pose_out is then inverse(T) of an unchanged T, not pose_in bit for bit).  pose_out[i] is pose_in[i] bit for bit when ns < 6 or
 * fewer than 6 correspondences were found at the first evaluation, with max_iteration 0 and below min_fitness; a class whose
 * normals_table entry is 0 is treated like one with M < 1.
 * APE_EINVAL as ape_icp_polish_batch_f64, and for a null normals_table. */
int ape_icp_polish_plane_batch_f64(int n, const float* points4, const int* n_cand, int N, const int* obj_class, const int64_t* model_table,
                                   const int64_t* normals_table, int n_classes, int max_model_points, double cell, const double* pose_in,
                                   double max_dist, double relative_fitness, double relative_rmse, int max_iteration, double min_fitness,
                                   double* pose_out, double* stats, void* stream);

/* ape_conv3x3_halo_bf16 for a 64-channel layer (the segmentor's up_3, pspnet.py:51) with ape_seg_head_f32 fused into its
 * epilogue: the [B][H][W][64] activation is never written, label[B][H][W] u8 / score[B][H][W] f32 are (bit-identical to the
 * unfused pair).  params->Cout must be 64, no residual; params->ups as in ape_conv3x3_halo_bf16. */
int ape_conv3x3_halo_seghead_bf16(const float* x, const void* w_packed, const float* bias, const ape_conv_params* params, int nsplit,
                                  const float* head_w, const float* head_b, int C, uint8_t* label, float* score, int double_softmax,
                                  void* stream);

/* ---- smp Unet decoder (segmentation_models_pytorch 0.1.3, restated in autoposeestimation_amd/segmentation/unet.py) ---------------
 * Replaces, in the Unet the reference builds at label_generator/create_labels.py:20-37, background_subtraction/utils.py:648-663 and
 * segmentation/__init__.py:252-256 (smp.Unet(encoder_name='resnet34')), smp's DecoderBlock.forward
 *     x = F.interpolate(x, scale_factor=2, mode='nearest'); x = torch.cat([x, skip], dim=1); x = conv1(x); x = conv2(x)
 * (each conv = Conv2d 3x3 p1 no bias + BatchNorm2d + ReLU, the BN folded into the weights and bias by the caller) and the
 * SegmentationHead (Conv2d 3x3 p1 + activation), on the bf16 matrix cores (nsplit 3 = split-bf16, 1 = plain bf16; fp32 accumulate).
 * The conv reads the VIRTUAL input cat([nearest_up2(a), b]): channel c < C1 of output pixel (y, x) is a[(y >> ups, x >> ups), c]
 * (a: [B][H >> ups][W >> ups][lda]), channel C1 + c is b[(y, x), c] (b: [B][H][W][ldb], C2 = 0: no skip, b may be null);
 * nothing up-sampled or concatenated is written.  H, W = the OUTPUT size (even when ups = 1).  w_packed = ape_pack_weights_bf16 of
 * the [Cout][3][3][C1 + C2] weights (K = 9 (C1 + C2), [tap][C1 | C2] order).  C1, C2, Cout multiples of 16 (C1 >= 16).
 * Offsets are 64-bit: no batch limit.  ape_unet_conv3x3_supported says whether a layer's channel counts are taken. */
int ape_unet_conv3x3_supported(int C1, int C2, int Cout, int ups);
/* y[b][y][x][yoff + co] = relu(conv + bias[co]) (fp32 NHWC, ldy % 4 == 0, yoff % 4 == 0). */
int ape_unet_conv3x3_bf16(const float* a, int lda, int C1, const float* b, int ldb, int C2, const void* w_packed,
                          const float* bias, float* y, int ldy, int yoff, int B, int H, int W, int Cout, int ups, int nsplit,
                          void* stream);
/* The segmentation head with the reference's post-processing fused (pipeline/utils.py:429-435): logits = conv + bias (C <= 16
 * classes, w_packed [C][3][3][C1 + C2]), then softmax (+ the second softmax when double_softmax) and arg-max by csrc/seg_head.h --
 * the same tie rule and score formula as ape_seg_head_f32 -- written as label[B][H][W] u8 and score[B][H][W] f32; the logits are
 * never stored. */
int ape_unet_conv3x3_seghead_bf16(const float* a, int lda, int C1, const float* b, int ldb, int C2, const void* w_packed,
                                  const float* bias, int C, uint8_t* label, float* score, int B, int H, int W, int ups, int nsplit,
                                  int double_softmax, void* stream);
/* F.interpolate(x, scale_factor=2, mode='nearest') (smp DecoderBlock, the materialised route; scale 1: a plain copy, for the skip half):
 * x[B][h][w][C] -> y[B][scale h][scale w][ldy] channels yoff .. yoff + C - 1 (C, ldy, yoff multiples of 4), i.e. straight into one
 * channel window of the concatenation buffer. */
int ape_nearest_upsample_nhwc_f32(const float* x, float* y, int B, int h, int w, int C, int scale, int ldy, int yoff, void* stream);


/* ---- training step: the backward kernels behind DenseFusion/tools/train.py:205-238 -------------------
 * `loss.backward()` / `dis.backward()` there run torch autograd over cuDNN; each entry below is one backward rule of the ops
 * the estimator / refiner / losses are built from (DenseFusion/lib/{network,pspnet,extractors,loss,loss_refiner}.py). */
/* Convolution weight gradient (nn.Conv2d / Conv1d / Linear backward w.r.t. weight): x, dy NHWC as in ape_conv2d_nhwc_f32 with
 * the same ape_conv_params; dw[Cout][KH][KW][Cin] in the packed forward layout (Cin % 4 == 0).  The input gradient is the
 * forward kernel applied to dy with the flipped, transposed weights. */
size_t ape_conv2d_wgrad_workspace_bytes(const ape_conv_params* params);
int ape_conv2d_wgrad_nhwc_f32(const float* x, const float* dy, float* dw, const ape_conv_params* params, void* workspace,
                              size_t workspace_bytes, void* stream);
/* the same sums written as the reference's parameter tensor: dw[Cout][cin_param][KH][KW] (cin_param <= Cin: the zero channels that pad x
 * to a multiple of 4 drop out) -- what `weight.grad` holds after train.py:221 */
int ape_conv2d_wgrad_param_f32(const float* x, const float* dy, float* dw, const ape_conv_params* params, int cin_param, void* workspace,
                               size_t workspace_bytes, void* stream);
/* dx = dy * act'(ref): ref = the OUTPUT for APE_ACT_RELU / APE_ACT_SIGMOID, the INPUT for APE_ACT_PRELU (nn.ReLU, nn.PReLU
 * pspnet.py:33, torch.sigmoid network.py:117); in place allowed */
int ape_act_bwd_f32(const float* dy, const float* ref, float* dx, long n, int act, float alpha, void* stream);
/* nn.PReLU with one slope (pspnet.py:33) as a separate op of the training forward, and its slope gradient
 * dalpha[0] = sum dy * x * [x <= 0]; scratch1024: 1024 floats */
int ape_prelu_f32(const float* x, float* y, long n, float alpha, void* stream);
int ape_prelu_dalpha_f32(const float* dy, const float* x, float* dalpha, long n, float* scratch1024, void* stream);
/* bias gradient: out[C] = column sums of x[rows][ld] at channel offset off; scratch: 64 * C floats */
int ape_colsum_f32(const float* x, float* out, long rows, int C, int ld, int off, float* scratch, void* stream);
/* nn.MaxPool2d(3, 2, 1) backward (extractors.py:91), ATen's first-maximum tie rule */
int ape_maxpool3x3s2_bwd_nhwc_f32(const float* x, const float* dy, float* dx, int B, int H, int W, int C, void* stream);
/* nn.AdaptiveAvgPool2d((S, S)) backward (pspnet.py:16) */
int ape_adaptive_avgpool_bwd_nhwc_f32(const float* dy, float* dx, int B, int H, int W, int C, int S, void* stream);
/* F.upsample(..., mode='bilinear') backward, both conventions of ape_bilinear_nhwc_f32 (pspnet.py:22, :37) */
int ape_bilinear_bwd_nhwc_f32(const float* dy, float* dx, int B, int H, int W, int C, int Ho, int Wo, int align_corners,
                              void* stream);
/* nn.LogSoftmax backward per row (pspnet.py:55) */
int ape_log_softmax_bwd_rows_f32(const float* dy, const float* y, float* dx, long rows, int C, void* stream);
/* torch.gather backward (network.py:100-102): dx[B][rows_in][C] = scatter-add of dy[B][n][C] at index[B][n]; an index outside
 * 0..rows_in-1 is clamped as ape_gather_rows_f32 clamps it (the adjoint of that forward) */
int ape_scatter_add_rows_f32(const float* dy, const int64_t* index, float* dx, int B, int rows_in, int n, int C, void* stream);
/* AvgPool1d(num_points) backward (network.py:64): dx[B][n][C] = dy[B][C] / n */
int ape_mean_rows_bwd_f32(const float* dy, float* dx, int B, int n, int C, void* stream);
/* Gradient of Loss (full = 1; loss.py:50-53) or of Loss_refine's dis (full = 0; loss_refiner.py:47) w.r.t. pred_r[N][4],
 * pred_t[N][3] (and pred_c[N]); dis / stdv from ape_adds_dis_f32, gscale = DEVICE scalar upstream gradient */
int ape_adds_grad_f32(const float* pred_r, const float* pred_t, const float* points, const float* model, const float* target,
                      const float* pred_c, const float* dis, const float* stdv, const float* gscale, int N, int M, int symmetric,
                      int full, float w, float* d_r, float* d_t, float* d_c, void* stream);
/* optim.Adam(lr) update of one flat parameter buffer (train.py:109,113; torch defaults betas (0.9, 0.999), eps 1e-8) */
int ape_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                      float beta2, float eps, int step, float weight_decay, void* stream);

/* The same update for n parameter buffers at once (64 per launch): optimizer.step() of train.py:231-232 over all parameters of the
 * estimator / refiner.  bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step) of each buffer's own step count. */
typedef struct ape_adam_job {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long n;
    float bc1, bc2_sqrt;
} ape_adam_job;
int ape_adam_step_multi_f32(int n, const ape_adam_job* jobs_host, float lr, float beta1, float beta2, float eps, float weight_decay,
                            void* stream);
/* After an optimizer step the conv kernels' weight operands are stale: one launch re-packs many parameters ([Cout][Cin][taps] f32, the
 * reference's nn.Conv2d / Conv1d / Linear layout) into f32 [N][taps][C4] (C4 = C rounded up to 4, zero channels) and, when dst_bf16 is
 * set, the split-bf16 planes of ape_pack_weights_bf16.  transpose = 0: N = Cout, C = Cin (forward operand); 1: N = Cin, C = Cout, taps
 * reversed (the flipped, transposed weights whose forward conv is the input gradient).  jobs: DEVICE array. */
typedef struct ape_pack_job {
    const float* src;
    float* dst_f32;
    void* dst_bf16;
    int cout, cin, taps, transpose;
    int src_ld;            /* elements between two output-channel rows of src (cin * taps when src is the whole parameter; larger for a
                              column block of a wider one, network.py:104-121 feeds conv1_r/t/c two column blocks of one weight) */
    int reserved;
} ape_pack_job;
int ape_pack_train_weights(int n, const ape_pack_job* jobs_device, long max_elems, void* stream);

/* ---- Segmentor training (csrc/segtrain.hip; reference segmentation/__init__.py:134-156 over smp 0.1.3's Unet) ----------------------
 * BatchNorm2d in train mode over x[rows][C] (rows = B*H*W, NHWC): mean[2 * C] (the batch mean as a float pair hi[C], lo[C]) and invstd[C]
 * (biased variance, eps) of the batch, running_mean /
 * running_var updated with `momentum` (unbiased variance, rows / (rows - 1)), num_batches_tracked[0] += 1 (i64; the three may be NULL),
 * then y = act((x - mean) * invstd * gamma + beta [+ residual]), act = APE_ACT_NONE | APE_ACT_RELU.  rows < 2 is refused (torch raises).
 * Workspace: ape_bn_workspace_bytes(C) for the forward, that plus 2 * C floats for the backward.  Deterministic (fixed-order partials). */
size_t ape_bn_workspace_bytes(int C);
int ape_bn_train_fwd_f32(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* mean, float* invstd,
                         float* running_mean, float* running_var, long long* num_batches_tracked, long rows, int C, float eps, float momentum,
                         int act, void* ws, size_t ws_bytes, void* stream);
/* Backward of the above: g = dy, masked by y > 0 when the saved output y is given (ReLU); dres = g (residual gradient, may be NULL),
 * dbeta = sum g, dgamma = sum g * x_hat, dx = gamma * invstd * (g - mean(g) - x_hat * mean(g * x_hat)) (dx / dgamma / dbeta may be NULL) */
int ape_bn_train_bwd_f32(const float* dy, const float* y, const float* x, const float* mean, const float* invstd, const float* gamma,
                         float* dx, float* dgamma, float* dbeta, float* dres, long rows, int C, void* ws, size_t ws_bytes, void* stream);
/* F.interpolate(scale_factor=2, mode='nearest') backward: dx[B][h][w][C] = 2x2 sums of dy[B][2h][2w][ld] channels off..off+C */
int ape_upsample_nearest2x_bwd_f32(const float* dy, int ld, int off, float* dx, int B, int h, int w, int C, void* stream);
/* softmax over the last (channel) axis of x[rows][C] and its backward dx = y * (dy - sum(dy * y)) */
int ape_softmax_rows_f32(const float* x, float* y, long rows, int C, void* stream);
int ape_softmax_rows_bwd_f32(const float* dy, const float* y, float* dx, long rows, int C, void* stream);
/* jaccard_loss(true, logits, eps) of segmentation/utils.py:71-114: logits[B][C][H][W] at element strides strides_host[4] (a channels-last
 * view is read in place), labels i64 [B*H*W], C in 1..32 (C == 1: the sigmoid pair with the swapped one-hot).  ncol = 1: intersections
 * and cardinalities summed over (B, H, W) (the reference's [B,1,H,W] labels); ncol = W: over (B, H) per column (its [B,H,W] labels, whose
 * reduction dims are (0, 2)).  loss[0] = 1 - mean over the label values present (and the columns) of I/(S - I + eps); NaN when a label is
 * outside the classes.  The workspace keeps the per-class terms the backward reads: pass the same one to ape_jaccard_bwd_f32, which writes
 * dlogits (at dstrides_host) times the device scalar gscale[0]. */
size_t ape_jaccard_workspace_bytes(int C, int ncol);
int ape_jaccard_fwd_f32(const float* logits, const long* strides_host, const long long* labels, int B, int C, int H, int W, int ncol,
                        float eps, float* loss, void* ws, size_t ws_bytes, void* stream);
int ape_jaccard_bwd_f32(const float* logits, const long* strides_host, const long long* labels, int B, int C, int H, int W, int ncol,
                        const float* gscale, float* dlogits, const long* dstrides_host, const void* ws, size_t ws_bytes, void* stream);
/* ConfusionMatrix.add of segmentation/utils.py:151-191: prediction and target each either scores[B][K][H][W] (strides_host; arg-max, first
 * maximum) or i64 labels [B*H*W] (exactly one of the two non-NULL); conf[K][K] u64 (rows = target, columns = prediction) accumulated with
 * integer atomics; bad_flag[0] |= 1 when a class falls outside 0..K-1 (that pixel is not counted).  K <= 64. */
int ape_confusion_add(const float* pred_scores, const long* pred_strides_host, const long long* pred_labels, const float* tgt_scores,
                      const long* tgt_strides_host, const long long* tgt_labels, int B, int H, int W, int K, unsigned long long* conf,
                      unsigned* bad_flag, void* stream);
/* torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov) over n parameter buffers (64 per launch): d = g + wd * p; buf = d on a
 * buffer's first step (first = 1), else momentum * buf + (1 - dampening) * d; d = nesterov ? d + momentum * buf : buf; p -= lr * d.
 * momentum_buffer may be NULL when momentum == 0. */
typedef struct ape_sgd_job {
    float* param;
    const float* grad;
    float* momentum_buffer;
    long n;
    int first;
    int reserved;
} ape_sgd_job;
int ape_sgd_step_multi_f32(int n, const ape_sgd_job* jobs_host, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                           void* stream);

/* ---- What the three training-sample builders below share: a rotation and an ordered list of colour ops, as the host drew them --------
 * ape_aug_rotation.  mode: APE_ROT_NONE, APE_ROT_180, APE_ROT_90 / APE_ROT_270 (Pillow's transposes, square frames only) or
 * APE_ROT_AFFINE = Pillow's Image.rotate through its AFFINE nearest-neighbour transform with zero fill: `a` is the inverse matrix
 * Image.rotate hands the transform (output pixel -> source position), read in double precision at the pixel centre by 16-bit images (the
 * depth), and `fa` its 16.16 fixed-point form FLOOR(v * 65536 + 0.5) of (a0, a1, a2 + a0/2 + a1/2, a3, a4, a5 + a3/2 + a4/2) that the
 * 8-bit images (RGB, label) walk.
 * ape_aug_jitter.  The first n_ops (<= 4) entries are ops APE_JIT_* in the order they run: brightness / contrast / saturation blend
 * towards black / the rounded mean of L over the whole image as it is at that point / L by `factor` (C float, truncated, clipped outside
 * [0, 1]); hue adds `shift` (0..255) to H of Pillow's HSV, wrapping.  At most one contrast per list. */
enum { APE_ROT_NONE = 0, APE_ROT_180 = 1, APE_ROT_AFFINE = 2, APE_ROT_90 = 3, APE_ROT_270 = 4 };
enum { APE_JIT_END = 0, APE_JIT_BRIGHTNESS = 1, APE_JIT_CONTRAST = 2, APE_JIT_SATURATION = 3, APE_JIT_HUE = 4 };
typedef struct ape_aug_rotation {
    double a[6];
    int fa[6];
    int mode;
    int reserved;
} ape_aug_rotation;
typedef struct ape_aug_jitter {
    int n_ops;
    int code[4];
    float factor[4];
    int shift[4];
} ape_aug_jitter;
APE_STATIC_ASSERT(sizeof(ape_aug_rotation) == 80, "ape_aug_rotation layout (mirrored by _lib.AugRotation)");
APE_STATIC_ASSERT(sizeof(ape_aug_jitter) == 52, "ape_aug_jitter layout (mirrored by _lib.AugJitter)");

/* ---- Background-subtraction training samples (csrc/bgsub_train.hip; reference background_subtraction/utils.py:414-646 load_subtraction +
 * augment, dataset.py:60-86) ---------------------------------------------------------------------------------------------------------
 * One job per sample of the batch: DEVICE pointers to the raw frames (any frames of a resident set: a batch is a table of pointers, not a
 * copy) and the augmentation the host drew.  Order per image: rotate (the RGB and the label walk `fa`, the depths read `a`) -> colour
 * jitter (RGB only; jit[0] = foreground, jit[1] = background) -> h-flip -> v-flip. */
typedef struct ape_bgsub_train_job {
    const uint8_t* f_rgb;      /* [H][W][3] */
    const uint8_t* b_rgb;
    const uint16_t* f_depth;   /* [H][W] */
    const uint16_t* b_depth;
    const uint8_t* label;      /* [H][W] */
    ape_aug_rotation rot;
    ape_aug_jitter jit[2];
    int hflip, vflip;
} ape_bgsub_train_job;
APE_STATIC_ASSERT(sizeof(ape_bgsub_train_job) == 232, "ape_bgsub_train_job layout (mirrored by _lib.BgsubTrainJob)");
/* x8[B][H][W][8] f32 NHWC: |f - b| of RGB (3), of Pillow's HSV (3) and of the depth after `f_depth[b_depth == 0] = 0` then
 * `b_depth[f_depth == 0] = 0` (no distance gate), each cast to uint8 as numpy does (the depth difference wraps mod 256), / 255, then
 * (x - mean7) / std7 (HOST pointers); channel 7 = 0.  label[B][H][W] i64 in {0, 1} (non-zero -> 1).  u8_or_null[B][H][W][7] receives the
 * uint8 channels.  Two launches (the L sums of the contrast ops, then everything), none when B == 0; bit-reproducible.  The workspace
 * (ape_bgsub_train_workspace_bytes(B)) carries the sums between the two and must not be shared by batches in flight at once. */
size_t ape_bgsub_train_workspace_bytes(int B);
int ape_bgsub_train_samples(const ape_bgsub_train_job* jobs_host, int B, int H, int W, const float* mean7_host, const float* std7_host,
                            float* x8, long long* label, uint8_t* u8_or_null, void* ws, size_t ws_bytes, void* stream);

/* ---- Segmentor training samples (csrc/seg_train.hip; reference segmentation/dataset.py:88-112 with the transforms of
 * segmentation/utils.py:25-66 and CropAndZoom :361-487) -------------------------------------------------------------------------------
 * One job per sample: DEVICE pointers to the resident frame and its label and what the host drew.  Order, as the reference composes it:
 * colour jitter of the full frame -> Image.rotate of image and label (both are 8-bit, so both walk `fa`; `a` is not read) -> crop of the square crop_side x crop_side box at (crop_x, crop_y) of the rotated frame (zero
 * outside it, like Image.crop) -> resize to S x S, Pillow's BICUBIC for the image and NEAREST for the label -> ToTensor, Normalize; label
 * pixels != 0 become class_id. */
typedef struct ape_seg_train_job {
    const uint8_t* rgb;        /* [H][W][3] */
    const uint8_t* label;      /* [H][W] */
    ape_aug_rotation rot;
    ape_aug_jitter jit;
    int crop_x, crop_y, crop_side;
    int class_id;
} ape_seg_train_job;
APE_STATIC_ASSERT(sizeof(ape_seg_train_job) == 168, "ape_seg_train_job layout (mirrored by _lib.SegTrainJob)");
/* The workspace of a batch: [B][64] u64 luma partial sums | [B][64][5] i32 extent partials at ape_seg_train_extents_offset(B) | the
 * resize tables [B][14 * S] i32 at ape_seg_train_tables_offset(B).  One per stream; not shared by batches in flight at once. */
size_t ape_seg_train_workspace_bytes(int B, int S);
size_t ape_seg_train_extents_offset(int B);
size_t ape_seg_train_tables_offset(int B);
/* Launch A (replaces the host's `np.where(label == 255)` of segmentation/utils.py:450-462 and ImageStat of ImageEnhance.Contrast): per
 * sample 64 workgroups, each writing ONE partial of the integer L sum of the un-rotated frame as it is when its contrast op runs, and one
 * (min row, max row, min column, max column, count) of the ROTATED label's pixels == 255 (INT_MAX, -1, INT_MAX, -1, 0 when it saw none).
 * The caller reads the extent partials back, combines them (min / max / sum: exact whatever the schedule), draws the crop boxes and fills
 * crop_* before launch B.  crop_* and class_id are not read here. */
int ape_seg_train_stats(const ape_seg_train_job* jobs_host, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* Launch B: img[B][3][S][S] f32 (16-byte aligned), label[B][S][S] i64.  The tables of sample b, built by the caller in double as
 * Pillow's Resample.c / ImagingScaleAffine do and copied into the workspace: hmin[S], hk[S][5], vmin[S], vk[S][5] (first source index and
 * the five 2^22 fixed-point BICUBIC weights of every output column / row; unused weights 0), nx[S], ny[S] (NEAREST source column / row).
 * A pass is clip8((2^21 + sum pixel * k) >> 22), horizontal first, its u8 result feeding the vertical one.  Enlargement only:
 * crop_side > S is APE_EINVAL. */
int ape_seg_train_samples(const ape_seg_train_job* jobs_host, int B, int H, int W, int S, const float* mean3_host, const float* std3_host,
                          float* img, long long* label, void* ws, size_t ws_bytes, void* stream);
/* The un-augmented sample of mode 'test' (segmentation/dataset.py:98-112 without the augmentations): img[B][3][H][W] f32 = (rgb / 255 -
 * mean) / std, label[B][H][W] i64 = class_id where the label is != 0.  Only rgb, label and class_id of a job are read. */
int ape_seg_plain_samples(const ape_seg_train_job* jobs_host, int B, int H, int W, const float* mean3_host, const float* std3_host, float* img,
                          long long* label, void* stream);

/* ---- DenseFusion training samples (csrc/pose_train.hip; reference DenseFusion/datasets/myDatasetAugmented/dataset.py:158-326) ---------
 * One job per sample: DEVICE pointers to the resident colour frame, 16-bit depth and label, and what the host drew.  Order, as the
 * reference composes it (:204-214): colour jitter of the full frame -> Image.rotate of colour, label and depth (the 8-bit images walk `fa`,
 * the depth reads `a`) ->
 * the get_bbox crop [rmin, rmax) x [cmin, cmax) of the rotated frame -> `choose`, the back-projected cloud and the normalised crop.
 * The crop, the intrinsics (as C floats: numpy computes the cloud in float32), depth_scale, to_meter, add_noise / add_t (the translation
 * noise, double: numpy adds it in float64 and rounds once) and out_off (byte offset of the sample in the output block, a multiple of 16)
 * are read by launch B only. */
typedef struct ape_pose_train_job {
    const uint8_t* rgb;        /* [H][W][3] */
    const uint16_t* depth;     /* [H][W] */
    const uint8_t* label;      /* [H][W] */
    ape_aug_rotation rot;
    double add_t[3];
    long long out_off;
    ape_aug_jitter jit;
    int rmin, rmax, cmin, cmax;
    float ppx, ppy, fx, fy, depth_scale;
    int to_meter, add_noise;
} ape_pose_train_job;
APE_STATIC_ASSERT(sizeof(ape_pose_train_job) == 232, "ape_pose_train_job layout (mirrored by _lib.PoseTrainJob)");
/* The workspace of a batch: [B][64] u64 luma partial sums | at ape_pose_train_extents_offset(B): [B][64][4] i32 extent partials, then
 * [B][H] i32 row counts (one read-back covers both) | at ape_pose_train_tables_offset(B, H): [B][H] i32 exclusive row prefix, then
 * [B][N] i32 `sel` (one upload covers both).  One per stream; not shared by batches in flight at once. */
size_t ape_pose_train_extents_offset(int B);
size_t ape_pose_train_rows_offset(int B);
size_t ape_pose_train_tables_offset(int B, int H);
size_t ape_pose_train_sel_offset(int B, int H);
size_t ape_pose_train_workspace_bytes(int B, int H, int N);
/* bytes of one sample in the output block: choose[N] i64 | points[N][3] f32 | (at ape_pose_train_image_offset(N), a multiple of 16)
 * img[3][Hc][Wc] f32; the total is rounded up to a multiple of 16 */
size_t ape_pose_train_image_offset(int N);
size_t ape_pose_train_sample_bytes(int N, int Hc, int Wc);
/* Launch A over the full frames: per sample 64 workgroups, each writing ONE partial of the integer L sum of the un-rotated frame as it is
 * when its contrast op runs and one (min row, max row, min column, max column) of the ROTATED label's pixels == 255 (INT_MAX, -1, INT_MAX,
 * -1 when it saw none); and rows[b][y] = the number of VALID pixels of row y (rotated label == 255 and rotated depth != 0), each row
 * written once by the one wave that walked it.  No atomics, nothing to zero.  The crop and what follows it in a job are not read. */
int ape_pose_train_stats(const ape_pose_train_job* jobs_host, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* Launch B.  The caller has read extents and row counts back, set the crops (every labelled pixel lies inside get_bbox's crop, so the row
 * counts are in-crop counts), and copied into the workspace the exclusive prefix of every sample's row counts and sel[B][N]: the RANKS,
 * among the valid pixels in row-major order, that `choose` keeps.  Per sample, at out + out_off: choose[j] = the flat index inside the crop
 * of the valid pixel of rank sel[j] (row by the prefix, column by a ballot walk of that row; 0 and a zero point when no such pixel
 * exists), points[j] = its back-projection in float32 without fused multiply-adds (+ add_t in double, rounded once, when add_noise),
 * img = ((float)v - mean[c]) / std[c] of the jittered, rotated frame inside the crop, planar (mean3 / std3: HOST pointers).
 * A crop outside the frame, outside 40..480 x 40..640 or not a multiple of 40, a sample that does not fit out_bytes, out or out_off not
 * 16-byte aligned: APE_EINVAL, nothing launched. */
int ape_pose_train_samples(const ape_pose_train_job* jobs_host, int B, int H, int W, int N, const float* mean3_host, const float* std3_host,
                           void* out, size_t out_bytes, void* ws, size_t ws_bytes, void* stream);

/* ---- LineMOD samples (csrc/linemod.hip; reference DenseFusion/datasets/linemod/dataset.py:90-195) -------------------------------------
 * One job per sample: DEVICE pointers to the resident colour frame, 16-bit depth and label ([H][W][label_bands] u8; band 0 decides, as
 * `masked_equal(label, [255, 255, 255])[:, :, 0]` does) and what the host drew.  There is no rotation.  The crop [rmin, rmax) x [cmin, cmax)
 * comes from the host's get_bbox over `obj_bb` or over the largest-contour box below, so label pixels may lie OUTSIDE it: only pixels
 * inside the crop are counted and chosen.  cam_*: the camera constants as C floats (numpy computes the cloud in float32):
 * z = depth / cam_scale, x = (col - cam_cx) * z / cam_fx, y = (row - cam_cy) * z / cam_fy, then each / 1000.0f; add_t (double) is added in
 * float64 and rounded once when add_noise.  skip != 0: the sample has no valid pixel; launch C writes nothing for it. */
typedef struct ape_linemod_job {
    const uint8_t* rgb;        /* [H][W][3] */
    const uint16_t* depth;     /* [H][W] */
    const uint8_t* label;      /* [H][W][label_bands] */
    double add_t[3];
    long long out_off;
    ape_aug_jitter jit;
    int rmin, rmax, cmin, cmax;
    int label_bands, add_noise, skip, reserved;
    float cam_cx, cam_cy, cam_fx, cam_fy, cam_scale;
} ape_linemod_job;
APE_STATIC_ASSERT(sizeof(ape_linemod_job) == 160, "ape_linemod_job layout (mirrored by linemod/augment.py LinemodJob)");
/* Largest-contour box of `mask_to_bbox` (dataset.py:216-230 with cv2.findContours / boundingRect restated): per frame the 8-connected
 * components of label == 255 (labels_host: HOST array of B DEVICE pointers to one-band [H][W] u8 labels), per component its extents,
 * boxes[b] = (x, y, w, h) of the component with the largest w * h, ties to the component whose first pixel comes first in raster order,
 * zeros when the frame has none.  Integer min / max / compare only: identical whatever the schedule.  B * H * W < 2^31. */
size_t ape_linemod_box_workspace_bytes(int B, int H, int W);
int ape_linemod_boxes(const void* const* labels_host, int B, int H, int W, int* boxes, void* ws, size_t ws_bytes, void* stream);
/* The workspace of a batch of samples: [B][64] u64 luma partial sums | at ape_linemod_rows_offset(B): [B][H] i32 row counts (the one
 * read-back) | at ape_linemod_tables_offset(B, H): [B][H] i32 exclusive row prefix, then at ape_linemod_sel_offset(B, H): [B][N] i32 `sel`
 * (one upload covers both).  One per stream; not shared by batches in flight at once.  A sample's bytes in the output block are those of
 * ape_pose_train_image_offset / ape_pose_train_sample_bytes: choose[N] i64 | points[N][3] f32 | img[3][Hc][Wc] f32. */
size_t ape_linemod_rows_offset(int B);
size_t ape_linemod_tables_offset(int B, int H);
size_t ape_linemod_sel_offset(int B, int H);
size_t ape_linemod_workspace_bytes(int B, int H, int N);
/* Launch B: rows[b][y] = the number of pixels of row y inside [cmin, cmax) with label band 0 == 255 and depth != 0 for rmin <= y < rmax,
 * 0 for the other rows, each row written once by the wave that walked it; and per workgroup one partial of the integer L sum of the whole
 * frame as it is when its contrast op runs.  A crop outside the frame, outside 40..480 x 40..640 or not a multiple of 40, label_bands
 * outside 1..4, a workspace that is misaligned or too short (in all three entry points): APE_EINVAL, nothing launched. */
int ape_linemod_rows(const ape_linemod_job* jobs_host, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* Launch C, after the caller copied the exclusive row prefixes and sel[B][N] (the RANKS, among the valid in-crop pixels in row-major
 * order, that `choose` keeps) into the workspace.  Per sample without `skip`, at out + out_off: choose[j] = the flat in-crop index of the
 * valid pixel of rank sel[j] (0 and a zero point when there is none), points[j] its cloud point, img = ((float)v - mean[c]) / std[c] of
 * the jittered frame inside the crop, planar.  The refusals of launch B, and a sample that does not fit out_bytes, out or out_off not
 * 16-byte aligned: APE_EINVAL, nothing launched. */
int ape_linemod_samples(const ape_linemod_job* jobs_host, int B, int H, int W, int N, const float* mean3_host, const float* std3_host,
                        void* out, size_t out_bytes, void* ws, size_t ws_bytes, void* stream);

/* ---- YCB-Video samples (csrc/ycb.hip, csrc/ycb_px.h; reference DenseFusion/datasets/ycb/dataset.py:97-232, tools/eval_ycb.py:136-190) ----
 * ape_ycb_jitter: an ape_aug_jitter in 24 bytes, so that 16 jobs with three lists each still travel as kernel arguments: the ops in the
 * order they run, code 0 (APE_JIT_END) ends the list; shift is the u8 hue shift.
 * One job per sample: DEVICE pointers to the resident colour frame, 16-bit depth and one-band label (classes 0..21), and what the host
 * drew.  back_rgb (or null): the real frame a `data_syn` sample is composited onto.  front_rgb / front_label (both or neither): the
 * synthetic frame whose classes front_a, front_b occlude the object.  jit[0] / jit[1] / jit[2] jitter the frame / the background / the
 * front (an empty list = none).  A pixel is a MEMBER when label == obj and the front label is neither front_a nor front_b, and VALID when
 * its depth is != 0 as well.  Per crop pixel, in uint8 arithmetic that wraps modulo 256 as numpy's does (:150-167):
 *   v = jittered frame; with back_rgb: v = jittered background * (label == 0) + v; with a front, where the front label is front_a or
 *   front_b: v = jittered front; then x = (float)((double)v + noise) with noise (ws + noise_off: f64 [3][Hc][Wc] in the workspace;
 *   noise_off < 0 = none) or (float)v, and (x - mean[c]) / std[c].
 * The cloud is z = depth / cam_scale, x = (col - cam_cx) * z / cam_fx, y = (row - cam_cy) * z / cam_fy in float32; add_t (double) is
 * added in float64 and rounded once when add_noise.  win_*: the rows [win_r0, win_r1) and columns [win_c0, win_c1) ape_ycb_rows counts
 * in.  skip != 0: ape_ycb_samples writes nothing for the sample. */
typedef struct ape_ycb_jitter {
    uint8_t code[4];
    uint8_t shift[4];
    float factor[4];
} ape_ycb_jitter;
typedef struct ape_ycb_job {
    const uint8_t* rgb;          /* [H][W][3] */
    const uint16_t* depth;       /* [H][W] */
    const uint8_t* label;        /* [H][W] */
    const uint8_t* back_rgb;     /* [H][W][3] or null */
    const uint8_t* front_rgb;    /* [H][W][3] or null */
    const uint8_t* front_label;  /* [H][W] or null */
    double add_t[3];
    long long out_off;
    long long noise_off;
    ape_ycb_jitter jit[3];
    int rmin, rmax, cmin, cmax;
    int win_r0, win_r1, win_c0, win_c1;
    int obj, front_a, front_b, add_noise, skip, reserved;
    float cam_cx, cam_cy, cam_fx, cam_fy, cam_scale, reserved_f;
} ape_ycb_job;
APE_STATIC_ASSERT(sizeof(ape_ycb_jitter) == 24, "ape_ycb_jitter layout (mirrored by ycb/augment.py YcbJitter)");
APE_STATIC_ASSERT(sizeof(ape_ycb_job) == 240, "ape_ycb_job layout (mirrored by ycb/augment.py YcbJob)");
/* One (label, front label or null, depth) triple of ape_ycb_overlap: DEVICE pointers to [H][W] u8 / u8 / u16. */
typedef struct ape_ycb_pair {
    const uint8_t* label;
    const uint8_t* front_label;
    const uint16_t* depth;
} ape_ycb_pair;
/* table[p][a][f][d] (u32 [P][22][22][2], zeroed here): the number of pixels of triple p with label == a, front label == f (0 with a null
 * front) and d = (depth != 0); a pixel with a class above 21 on either side is counted nowhere.  Per workgroup 968 counters in LDS, then
 * one global integer add per non-zero counter: integers only, so two launches agree bit for bit.  The host derives from this one table
 * both the over-1000 test of a front candidate and every object's valid-pixel count after its occlusion.  A null or misaligned pointer:
 * APE_EINVAL, nothing launched and the table untouched. */
int ape_ycb_overlap(const ape_ycb_pair* pairs_host, int P, int H, int W, uint32_t* table, void* stream);
/* The workspace of a batch: [B][3][64] u64 luma partial sums (frame, background, front) | at ape_ycb_rows_offset(B): [B][H][3] i32 (the
 * read-back) | at ape_ycb_tables_offset(B, H): [B][H] i32 exclusive row prefix, at ape_ycb_sel_offset(B, H): [B][N] i32 `sel`, at
 * ape_ycb_noise_offset(B, H, N) (a multiple of 16): the f64 noise of the samples that have one, each at its job's noise_off (one upload
 * covers the three).  One per stream; not shared by batches in flight at once.  A sample's bytes in the output block are those of
 * ape_pose_train_image_offset / ape_pose_train_sample_bytes. */
size_t ape_ycb_rows_offset(int B);
size_t ape_ycb_tables_offset(int B, int H);
size_t ape_ycb_sel_offset(int B, int H);
size_t ape_ycb_noise_offset(int B, int H, int N);
/* One wave per frame row: rows[b][y] = (the VALID pixels of row y inside the job's window -- 0 for a row outside it --, the first and the
 * last column of the row's MEMBERS over the whole row: W and -1 when it has none); and per workgroup one partial of the integer L sum
 * that the contrast op of each of the three lists needs, over the whole image it jitters.  The crop, add_t, noise_off and out_off are not
 * read.  A window outside the frame, obj / front_a / front_b outside 1..21 (0..21 for the front classes without a front), a front with
 * only one of its two pointers, a null or misaligned pointer, a short workspace: APE_EINVAL, nothing launched. */
int ape_ycb_rows(const ape_ycb_job* jobs_host, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* After the caller copied prefixes, sel[B][N] (the RANKS among the VALID pixels in row-major crop order that `choose` keeps) and the noise
 * into the workspace.  Per sample without `skip`, at out + out_off: choose[j] = the flat in-crop index of the valid pixel of rank sel[j]
 * inside the crop (0 and a zero point when there is none), points[j] its cloud point, img the normalised planar crop.  The refusals of
 * ape_ycb_rows; a crop outside the frame, outside 40..480 x 40..640 or not a multiple of 40; noise_off not a multiple of 8 or its
 * 24 * Hc * Wc bytes not inside the workspace; a sample that does not fit out_bytes, out or out_off not 16-byte aligned: APE_EINVAL,
 * nothing launched. */
int ape_ycb_samples(const ape_ycb_job* jobs_host, int B, int H, int W, int N, const float* mean3_host, const float* std3_host, void* out,
                    size_t out_bytes, void* ws, size_t ws_bytes, void* stream);

/* ---- SegNet glue (csrc/segnet.hip): DenseFusion/vanilla_segmentation/segnet.py:74-121, loss.py:11-21 --------------------------------
 * All NHWC fp32, C % 4 == 0, 16-byte aligned maps (codes 4-byte aligned).  APE_EINVAL: a negative size, C % 4 != 0, more than 2^31
 * elements, a null or misaligned pointer to a non-empty buffer; APE_OK without a launch when there is nothing to write.
 *
 * F.max_pool2d(x, kernel_size=2, stride=2, return_indices=True): x[B][H][W][C] -> y[B][H/2][W/2][C] and code[B][H/2][W/2][C] (an odd
 * last row / column is dropped), code = 2 * dy + dx of the winner.  ATen's CPU rule: scan (0,0) (0,1) (1,0) (1,1) from -inf at position
 * 0 and take an element if `v > best || isnan(v)` -- the first of equal maxima, the last NaN. */
int ape_maxpool2x2_idx_nhwc_f32(const float* x, float* y, uint8_t* code, int B, int H, int W, int C, void* stream);
/* F.max_unpool2d(y, idx, 2, 2, output_size=(H, W)): EVERY element of x[B][H][W][C] is written -- y at the coded position of its window,
 * 0 at the other three and in an odd last row / column -- by the one thread that owns its window (no memset, no scatter).  Also the
 * backward of the pool above. */
int ape_max_unpool2x2_nhwc_f32(const float* y, const uint8_t* code, float* x, int B, int H, int W, int C, void* stream);
/* y[B][H/2][W/2][C] = the element of each 2x2 window of x[B][H][W][C] that code names: the backward of the unpool. */
int ape_gather2x2_nhwc_f32(const float* x, const uint8_t* code, float* y, int B, int H, int W, int C, void* stream);
/* nn.CrossEntropyLoss() (mean) over the P pixels of logits[P][ld], classes = channels 0..C-1 (1 <= C <= 64, C <= ld; channels
 * C..ld-1 are never read), labels[P] u8.  out[0] = mean over the VALID pixels (label < C) of logsumexp(x) - x[label] (maximum subtracted,
 * fp32 per pixel, summed in float64 in a fixed two-stage order: two launches agree bit for bit), out[1] = the number of pixels with a
 * label >= C, which add nothing to the loss or the gradient.  dlogits (may be NULL): dlogits[p][c] = g * (softmax - onehot) / n_valid,
 * channels C..ld-1 written 0.  Three launches with a gradient (terms + unscaled gradient, the mean, the scale), two without.
 * P == 0 is NOT a no-op: `out` must still be defined, so the mean and the count are written -- NaN (0 / 0, torch's mean over nothing)
 * and 0; dlogits is then untouched.  A short workspace: APE_EWORKSPACE. */
size_t ape_cross_entropy_workspace_bytes(long P);
int ape_cross_entropy_f32(const float* logits, int ld, int C, const uint8_t* labels, long P, float g, double* out, float* dlogits,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- SegNet training samples (csrc/segnet_samples.hip, csrc/segnet_px.h; reference DenseFusion/vanilla_segmentation/
 * data_controller.py:43-93) -------------------------------------------------------------------------------------------------------------
 * One job per sample: DEVICE pointers to the resident colour frame and one-band label and what the host drew.  back_rgb / back_label
 * (both or neither) make the job a `data_syn` one: the frame is brightened (ImageEnhance.Brightness: pil_blend(0, v, bright), 1.5 in the
 * reference), blurred -- Pillow's box blur of ImageFilter.GaussianBlur, three passes along the rows and then three along the columns of
 *   out = (c * blur_ww + (l + r) * blur_fw + 2^23) >> 24, stored as u8 after every pass, the end pixel standing in for a missing
 * neighbour -- and jittered by jit[0]; then, per pixel, v = (double)v + noise, v = (double)(jit[1](back_rgb) * (label == 0)) + v,
 * label' = back_label * (label == 0) + label in uint8.  noise: f64 [3][H][W] in the workspace at noise_off, in un-flipped coordinates;
 * blur_off: where the prepare launch leaves the blurred frame u8 [H][W][3] in the workspace.  A job without a background is a real frame:
 * jit[0] of the raw frame (an empty list = none) and its label.  flip: 0 left-right, 1 up-down, 2 both, 3 neither, applied last.
 * Output: rgb[c] = ((float)v - mean[c]) / std[c] on the 0..255 scale, target = label'. */
typedef struct ape_segnet_job {
    const uint8_t* rgb;          /* [H][W][3] */
    const uint8_t* label;        /* [H][W] */
    const uint8_t* back_rgb;     /* [H][W][3] or null */
    const uint8_t* back_label;   /* [H][W] or null */
    long long noise_off;
    long long blur_off;
    ape_aug_jitter jit[2];
    float bright;
    uint32_t blur_ww, blur_fw;
    int flip;
} ape_segnet_job;
APE_STATIC_ASSERT(sizeof(ape_segnet_job) == 168, "ape_segnet_job layout (mirrored by vanilla_segmentation/augment.py SegnetJob)");
/* The workspace of a batch: [B][2][64] u64 luma partial sums (frame, background) | from ape_segnet_samples_frames_offset(B) (a multiple
 * of 16) on, wherever the jobs' blur_off (a multiple of 16, H*W*3 bytes) and noise_off (a multiple of 8, 24*H*W bytes) say; the caller
 * keeps these regions apart.  One per stream; not shared by batches in flight at once. */
size_t ape_segnet_samples_frames_offset(int B);
/* Launch A: writes the blurred frame of every `data_syn` job and, per workgroup, one partial of the integer L sum the contrast op of
 * each list needs, over the image it jitters as it is when the op runs.  flip and noise_off are not read.  APE_EINVAL, nothing launched:
 * a null or half-given pointer, a list jitter_ok refuses, blur_ww + 2 * blur_fw above 2^24, a NaN bright, a blur_off that is misaligned
 * or whose frame does not lie inside the workspace behind the sums; a short workspace: APE_EWORKSPACE. */
int ape_segnet_samples_prepare(const ape_segnet_job* jobs_host, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* Launch B, after the caller copied the noise into the workspace: rgb[B][3][H][W] f32, target[B][H][W] i64.  The refusals of launch A;
 * a flip outside 0..3; a noise_off that is misaligned or whose planes do not lie inside the workspace behind the sums. */
int ape_segnet_samples(const ape_segnet_job* jobs_host, int B, int H, int W, const float* mean3_host, const float* std3_host, float* rgb,
                       long long* target, void* ws, size_t ws_bytes, void* stream);

/* ---- overlays of the live view and of the label-review screens (csrc/overlay.hip) -------------------------------------------------
 * Replaces the `color_prediction` painting of full_prediction, pipeline/utils.py:471-476 (class tint), :510-513 and :576-585 (model
 * cloud stamped at the predicted pose) with pc_reconstruction/open3d_utils.py:233-243 (points2pixel) and :246-270 (pointcloud2image);
 * and the arithmetic of visualise_segmentation_maks :280-286 and visualise_pose_label :357-362.
 *
 * Count planes: planes[J][B][H][W] u32; plane j of frame b belongs to the j-th object of that frame.
 *
 * Stamp counts.  objs_host[n][4] i32 (HOST) = (frame, first row, rows, plane) of each object: its model cloud is rows
 * first .. first+rows-1 of clouds[total_points][3] f64.  pose_form 0: pose[n][7] f64 (w,x,y,z,tx,ty,tz), R as
 * DenseFusion/lib/transformations.py:1254-1278 (quaternion_matrix); pose_form 1: pose[n][3][4] f64 row-major [R|t].  n_cand: NULL, or
 * n_cand[n] i32 -- an object with n_cand <= 0 stamps nothing.  The call first clears all J*B*H*W counts, then per model point, in
 * float64 with one rounding per multiply and add: p' = R.p + t (each row summed left to right), col = (long long) (x'/(z'/fx) + ppx),
 * row = (long long) (y'/(z'/fy) + ppy) (truncation toward zero, points2pixel's int()); with step = (point_size-1)/2 the centre counts
 * -- one integer atomic add -- only if row-step >= 0, col-step >= 0, row+step+1 <= H and col+step+1 <= W (the stamps that
 * pointcloud2image keeps).  Points with z' == 0 or a projected coordinate that is not finite or outside int32 are skipped.
 * APE_EINVAL, nothing enqueued: a null planes (or, with n > 0, objs_host / clouds / pose), point_size even or < 1, B, H, W or J <= 0,
 * B*H*W >= 2^31, a frame outside 0..B-1, a plane outside 0..J-1, first + rows beyond total_points, a misaligned pointer. */
int ape_overlay_stamp_counts_f64(const int32_t* objs_host, int n, const double* clouds, long total_points, const double* pose,
                                 int pose_form, const int32_t* n_cand, double fx, double fy, double ppx, double ppy, int point_size,
                                 uint32_t* planes, int J, int B, int H, int W, void* stream);
/* Blend.  rgb[B][H][W][3] u8 -> seg_out, pose_out of the same shape, every byte written, in one pass.  slot_obj[B][J] i32 = the object
 * that owns plane j of frame b, in painting order, or -1; obj_cls[n] i32 = the class whose pixels of objmap[B][H][W] u8 the object tints
 * (<= 0: none; objmap NULL: no tint at all); seg_colour[n][3] and mark[n][3] f64 = its tint and its stamp colour (NULL: (255,0,0), the
 * default of open3d_utils.py:251-255); n_cand as above: such an object is painted in neither image.
 *   seg_out:  v*0.7 + colour*0.3 where the pixel's class is a painted object's class of its frame, else the frame's pixel.
 *   pose_out: per object in plane order, k = its counts summed over the point_size x point_size neighbourhood of the pixel = the stamps
 *             covering it; v = (mark*0.3) + (v*0.7) applied k times (the loop leaves early only when an application returns its input
 *             bit for bit).
 * mode 0 (full_prediction): v stays float64 through all blends, clip(0,255) and truncation to u8 once at the end.  mode 1 (the review
 * screens, which blend into a uint8 array): v is truncated to u8 after every application; the tint likewise.
 * APE_EINVAL, nothing enqueued: a null rgb / slot_obj / planes / seg_out / pose_out (or, with n > 0, obj_cls), aliased images, point_size even or < 1,
 * B, H, W or J <= 0, an unknown mode, an image or table not aligned to its element (images: 4 bytes). */
int ape_overlay_blend_u8(const uint8_t* rgb, const uint8_t* objmap, const int32_t* slot_obj, const int32_t* obj_cls,
                         const double* seg_colour, const double* mark, const int32_t* n_cand, int n, const uint32_t* planes,
                         int J, int B, int H, int W, int point_size, int mode, uint8_t* seg_out, uint8_t* pose_out, void* stream);

/* ---- classical RGB-D labeller   label_generator/utils.py:45-364 (createLabel_RGBD), csrc/label_rgbd.hip ------------------------
 * A batch of frame pairs [B][H][W], float64 where the reference is.  Parity with OpenCV unpinned: cvtColor, morphologyEx, filter2D and
 * connectedComponents follow the documented semantics restated in tests/label_rgbd_reference.py.  B <= 65535, B H W < 2^31 - 64. */
#define APE_RGBD_MODE_RGB 0
#define APE_RGBD_MODE_HSV 1
#define APE_RGBD_MODE_BOTH 2
/* depth u16 -> out f64: the value inside [measure_dist[b] - 150, measure_dist[b] + 150], else 0 (:102-108) */
int ape_rgbd_gate_f64(const uint16_t* depth, const double* measure_dist, double* out, int B, int H, int W, void* stream);
/* the centre window rows r0..r1-1, columns c0..c1-1 of the gated background depth, in place (:135-159): holes take
 * norm of (row, col, Z) of the plane through pts[B][3][3] f64 = three (row, col, depth) window points, then the 5 x 5 box filter with
 * float32 taps and BORDER_REFLECT_101 over the window.  valid[B] i32 == 0 leaves the frame alone.  tmp: f64 [B][r1-r0][c1-c0]. */
int ape_rgbd_plane_fill_f64(double* b_depth, const double* pts, const int* valid, double* tmp, int B, int H, int W, int r0, int r1,
                            int c0, int c1, void* stream);
/* smoothing (:26-30): filter2D with ones((k, k), float32) / (k k), BORDER_REFLECT_101, the taps summed in row-major order; dst != src */
int ape_rgbd_box_f64(const double* src, double* dst, int B, int H, int W, int k, void* stream);
/* the score (:179-251) in one pass: channel differences (HSV through OpenCV's 8-bit integer formula), hue times 256/180, clip at 100,
 * weights7_host[0..5] per channel, summed left to right -> color; plus the clipped depth difference times weights7_host[6] when that
 * is > 0 (f_depth is gated here, b_depth is the prepared f64 frame, the mutual zeroing of :165-166 happens per pixel); values below
 * threshold become 0 -> score.  Without a depth term f_depth, b_depth and measure_dist may be NULL. */
int ape_rgbd_score_f64(const uint8_t* f_rgb, const uint8_t* b_rgb, const uint16_t* f_depth, const double* b_depth,
                       const double* measure_dist, int mode, const double* weights7_host, double threshold, double* score,
                       double* color, int B, int H, int W, void* stream);
/* erode (dilate == 0) or dilate with a k x k all-ones kernel anchored at k / 2: min / max over offsets -(k/2) .. k-1-(k/2) of the
 * in-image pixels, rows then columns.  dst may be src; tmp (same size) may be neither. */
int ape_rgbd_morph_f64(const double* src, double* dst, double* tmp, int B, int H, int W, int k, int dilate, void* stream);
/* np.array(img, dtype=np.uint8) of a non-negative image: truncate toward zero, wrap modulo 256 */
int ape_rgbd_wrap_u8(const double* img, uint8_t* out, long npix, void* stream);
size_t ape_rgbd_cca_workspace_bytes(int B, int H, int W);
/* 8-connected components of the wrapped image's non-zero pixels: root[p] = the batch-wide index of the component's first pixel in
 * raster order (-1: background); at those pixels count = the component's size and sum = the sum of img over it (elsewhere 0).  The sum
 * is accumulated in integer fixed point (2^-52 units): it does not depend on the order of arrival. */
int ape_rgbd_component_stats(const double* img, int* root, unsigned int* count, double* sum, int B, int H, int W, void* workspace,
                             size_t workspace_bytes, void* stream);
/* one component round (:271-315 with by_size == 0, :330-355 with by_size == 1): among the components of img with more than min_size
 * pixels the one with the largest int(mean of img) or the largest size wins, strict '>' in raster order; without a winner the
 * reference's uni[0] is kept: the background region, or everything when no pixel is background.  color is zeroed outside the kept
 * label in place; remove_one_std then zeroes its pixels below mean - std of its non-zero pixels (mean_std_or_null[B][2] receives the
 * two).  With out_or_null the final mask (255 where the kept colour score is non-zero) is written instead and color is left alone. */
int ape_rgbd_cca_round(const double* img, double* color, uint8_t* out_or_null, double* mean_std_or_null, int B, int H, int W,
                       int min_size, int by_size, int remove_one_std, void* workspace, size_t workspace_bytes, void* stream);

/* ---- label-quality audit   experiments/gt_test.py (compute_IoU :160-194, the comparison image :105-120), csrc/label_audit.hip -------
 * labels: u8 [B][L][HW], L label planes per sample, densely packed: plane p of sample b starts at byte (b L + p) HW, whatever its
 * alignment.  A pixel is foreground when its byte is not zero.  B L HW < 2^31. */
/* counts u64 [B][P][4] for the P plane pairs pairs_host[P][2] = (a, b) of every sample, in the reference's order and under its names:
 * a fg and b fg ("tp"), a fg and b bg ("fp"), a bg and b fg ("fn"), both bg ("tn") -- the four values 0, 1, 2, 3 of its uint8
 * difference; "fp" and "fn" are swapped against the textbook meaning when a is the ground truth, which is restated, not corrected.
 * One pass: every plane is read once and serves all pairs.  counts (8-byte aligned) is cleared on the stream first and every entry is
 * written: a second call overwrites.  Integer sums, exact and independent of the order of arrival.  1 <= L <= 8, 1 <= P <= 16;
 * APE_EINVAL (nothing enqueued) for a null pointer, a size out of range, a pair index outside 0..L-1 or a misaligned counts. */
int ape_label_pair_counts_u8(const uint8_t* labels, int B, int L, int HW, const int32_t* pairs_host, int P, uint64_t* counts,
                             void* stream);
/* out u8 [B][H][W][3] = rgb, then where labels[plane_a] != 0: out[ch_a] = u8(trunc(double(out[ch_a]) c0 + double(label_a) c1)), then
 * the same with plane_b and ch_b on what the first step left (it matters when ch_a == ch_b).  float64, the product and the sum rounded
 * separately; a result outside 0..255 wraps modulo 256 (unpinned: the reference's c0 + c1 = 1 keeps it inside).  Every byte of out is
 * written.  APE_EINVAL for a null pointer, out overlapping rgb, a channel outside 0..2, a plane outside 0..L-1, a size below 1. */
int ape_label_pair_blend_u8(const uint8_t* rgb, const uint8_t* labels, int B, int L, int H, int W, int plane_a, int ch_a, int plane_b,
                            int ch_b, double c0, double c1, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* APE_HIP_H */
