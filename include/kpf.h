/*
 * kpf.h — C ABI of libkpf_hip.so, the MI355X (gfx950) compute library behind keypointfusion_amd.
 *
 * The reference (ru1ven/KeypointFusion) is pure Python on PyTorch: it has no FFI of its own, its "operators" are
 * the nn.Module forwards listed below, and the native code it reaches is cuDNN/cuBLAS/ATen/pointnet2_ops
 * (SURVEY.md §2.1).  Each entry point here replaces the native work behind one such forward, on raw device
 * pointers (fp32, 16-byte aligned) and a hipStream_t passed as void*.  No torch type crosses this boundary; the
 * Python host (keypointfusion_amd/model/model.py) owns memory through torch's caching allocator and passes
 * data_ptr()s.  All activations are NHWC ("pixel-major, channels contiguous"), optionally a channel slice
 * [coff, coff+C) of a wider buffer with pixel stride ld (this is how torch.cat along channels is made free).
 *
 * Every function returns 0 on success or a negative KPF_E* code; kpf_last_error() gives the thread-local message
 * (the Python side raises RuntimeError with it, mirroring the reference's Python-exception error convention).
 * Nothing here allocates, synchronises or touches the default stream: launches are graph-capturable.
 */
#ifndef KPF_H
#define KPF_H

#ifdef __cplusplus
extern "C" {
#endif

#define KPF_OK 0
#define KPF_EINVAL (-1)  /* bad shape / alignment / flag combination */
#define KPF_ELAUNCH (-2) /* HIP launch error */

/* Activation / weight storage types of the reduced-precision path (entry points ending in _h16): fp32 accumulation and fp32
 * elementwise arithmetic everywhere, 16-bit storage in HBM, v_mfma_f32_16x16x32_{bf16,f16} for the GEMMs. */
#define KPF_DT_F32 0
#define KPF_DT_BF16 1
#define KPF_DT_F16 2
/* kpf_conv2d_wgrad only (ABI 17): fp32 operands, the products taken on their bf16 / f16 roundings (16-bit MFMA, fp32 accumulation) — the weight
 * gradient of a layer whose forward ran with KPF_MMA_BF16 / _F16; honoured by the 64 x 64 tile form, fp32 products otherwise */
#define KPF_DT_F32_MMA_BF16 8
#define KPF_DT_F32_MMA_F16 9

/* kpf_conv_desc.flags */
#define KPF_ACT_RELU 1u        /* y = relu(acc + bias)                                    */
#define KPF_ACT_GELU 2u        /* y = gelu_erf(acc + bias)        (convNeXT/convnext.py:33) */
#define KPF_RES_ADD 4u         /* y = res + y                                              */
#define KPF_RES_GAMMA 8u       /* y = res + gamma[n] * y          (convNeXT/convnext.py:48-51) */
#define KPF_RELU_AFTER_RES 16u /* y = relu(res + y)               (model/resnet.py:72-73)  */
#define KPF_ACT_LEAKY 64u      /* y = leaky_relu(acc + bias, 0.01) (model/mano_head.py:199) */
#define KPF_IN_SPLIT 128u      /* `in` and `w` are in the split format below; needs a dense 1x1, Cin % 32 == 0, desc.w_unscale   */
#define KPF_W_SPLIT 512u       /* only `w` is split: fp32 activations are split in registers (any conv shape with Cin % 32 == 0)  */
#define KPF_OUT_SPLIT 256u     /* `out` is written in the split format (N, out_ld, out_coff multiples of 32)                     */
#define KPF_OUT_NCHW 32u       /* store out[b][n][oy][ox] (dense), ignoring out_ld/out_coff */
#define KPF_ACT_GELU_SAVE 2048u /* with KPF_ACT_GELU (ABI 13): also store the pre-activation acc + bias to the buffer passed in the `res` slot (res_ld / res_coff describe
                                  it; no residual is read) and use the exact erf GELU — the forward of a training Linear + GELU in one launch */
#define KPF_MMA_BF16 8192u     /* kpf_conv2d_f32 (ABI 17): fp32 storage, but the products MAY take the operands rounded to bf16 in registers (16-bit MFMA, fp32 accumulation) —
                                  what torch.autocast does to a Linear between fp32 tensors; honoured by the plain 1x1 / linear launches of the 256 x 128, 128 x 128 and
                                  128 x 64 tiles (the fusion head's wide Linears in the mixed-precision training step), ignored elsewhere */
#define KPF_MMA_F16 16384u     /* the same with f16 rounding */
#define KPF_PRO_LN 4096u       /* kpf_conv2d_h16 with KPF_ACT_GELU (ABI 15): the LayerNorm in front of the layer (convNeXT/convnext.py:42-44, pwconv1(norm(x))) is folded
                                  into the GEMM: `in` is the un-normalised tensor, `w` holds W diag(ln_w), `bias` W ln_b + b, pro_shift s[n] = sum_k w[n][k] (of the
                                  16-bit weights, in fp32) and pro_scale the (mean, rstd) pair of every pixel (kpf_ln_stats_merge);
                                  out = gelu(rstd * (acc - mean * s[n]) + bias[n]).  Layers gemm16_8ph_kernel covers only (kpf_conv2d_h16_uses_8ph) */
#define KPF_RES_GELU_GRAD 1024u /* with KPF_RES_ADD (ABI 13): y = (acc + bias) * gelu'(res) instead of the sum — the data gradient of Linear(gelu(z)) towards z
                                  in the GEMM's epilogue, res = z (training step: pwconv2 / output.dense backward; dense 1x1 only) */

typedef struct kpf_conv_desc {
  int B, IH, IW, Cin;      /* input: B x IH x IW pixels, Cin channels consumed per pixel            */
  int in_ld, in_coff;      /* floats between consecutive input pixels; first consumed channel       */
  int OH, OW, N;           /* output: B x OH x OW pixels, N channels                                */
  int KH, KW, sh, sw, ph, pw; /* filter taps, strides, zero padding                                 */
  int Kp;                  /* packed weight row length: >= KH*KW*Cin, multiple of 32, zero padded   */
  int out_ld, out_coff;    /* NHWC destination pixel stride / first channel                         */
  int res_ld, res_coff;    /* residual source (NHWC) pixel stride / first channel                   */
  unsigned flags;
  float w_unscale;         /* split operands only: weights were packed as w * 2^s, the accumulator is scaled by 2^-s */
  int tile_cfg;            /* 0: tile shape chosen by the built-in cost model; i+1: use configuration i < kpf_conv_num_tile_cfgs()
                              (the host side times the candidates once per shape and passes the fastest) */
  int groups;              /* 0 / 1: one convolution.  G > 1 (ABI 13): G independent convolutions of this shape in ONE launch (grid.y = group) —
                              group g consumes input channels [in_coff + g*Cin, +Cin) of the same pixels, multiplies by the weights at
                              w + g*w_gstride (bias[g*N + n]) and writes output channels [out_coff + g*N, +N): a grouped convolution over
                              channel-stacked activations.  The training step runs the depth and the RGB backbone (same architecture, two weight
                              sets: model/model.py:287-306) this way; a residual is stacked like the output (res_coff + g*N); no layer scale /
                              prologue / NCHW / split operands in a grouped launch. */
  long w_gstride;          /* elements between the groups' packed weight matrices (multiple of 4; 8 for 16-bit weights) */
} kpf_conv_desc;

/*
 * Implicit-GEMM convolution / linear layer on fp32 MFMA (v_mfma_f32_16x16x4_f32):
 *     out[m][n] = epilogue( sum_k A[m][k] * W[n][k] + bias[n] ),  m = (b,oy,ox),  k = (ky,kx,c) with c fastest,
 *     A[m][k]  = prologue( in[b][oy*sh+ky-ph][ox*sw+kx-pw][c] ), zero outside the image,
 *     prologue(x) = relu(x * pro_scale[c] + pro_shift[c]) when pro_scale != NULL (eval BatchNorm + ReLU on the operand).
 * Replaces: nn.Conv2d / nn.Linear / nn.Conv1d(k=1) forwards reached from model/hourglass.py:64-119 (Conv, Residual),
 * convNeXT/convnext.py:31-34,77,84 (pwconv1/2, stem, downsample), model/resnet.py:52-55,166 (BasicBlock, stem),
 * convNeXT/resnetUnet.py:95-97 (finals) — i.e. cuDNN implicit GEMM + cuBLAS sgemm in the reference.
 * w is [N][Kp] (PyTorch [out][in] order, taps reordered to (ky,kx,c)); bias may be NULL.
 * Requirements: Cin, in_ld, in_coff multiples of 4.  out/res ld and coff multiples of 4 select the float4 epilogue
 * (scalar stores otherwise).
 *
 * Split operands (KPF_IN_SPLIT / KPF_OUT_SPLIT): fp32-accurate GEMM on the f16 matrix cores.  A row of C values (C % 32 == 0)
 * keeps its C*4 bytes but holds, per 32-channel block, [32 x f16 hi | 32 x f16 lo] with x ~= hi + lo (22 significant bits).
 * With KPF_IN_SPLIT both `in` and `w` (rows of Kp) are in that format and each 32-deep K tile is 3 v_mfma_f32_16x16x32_f16
 * (hi*hi + hi*lo + lo*hi) accumulated in fp32: per-product error ~2^-21, below the rounding noise of an fp32 accumulation chain,
 * at 3/16 of the f32-input MFMA's cycles.  Weights are packed as w * 2^s (keeps the lo halves out of the f16 subnormals) and
 * desc.w_unscale = 2^-s.  With KPF_W_SPLIT only the weights are pre-split: activations stay fp32 in memory and are split in registers
 * after the LDS read (and after the operand prologue), at some VALU cost per fragment.  Producers of split activations: this function with KPF_OUT_SPLIT, kpf_layernorm_split_f32,
 * kpf_dwconv7_ln_split_f32.  Values are clamped to +-65504 when split; callers bound their activations (LayerNorm / GELU outputs).
 */
int kpf_conv2d_f32(const kpf_conv_desc* d, const float* in, const float* w, const float* bias,
                   const float* pro_scale, const float* pro_shift, const float* gamma, const float* res,
                   float* out, void* stream);

/*
 * ConvNeXt block front half: depthwise 7x7 (pad 3) + bias, then LayerNorm over channels (eps), fused.
 * x, y: dense NHWC [B][H][W][C]; w_dw: [49][C] (tap-major); replaces convNeXT/convnext.py:41-43
 * (cuDNN depthwise conv + permute + ATen layer_norm).  C % 4 == 0, C <= 2048.
 */
int kpf_dwconv7_ln_f32(const float* x, const float* w_dw, const float* b_dw, const float* ln_w, const float* ln_b,
                       float* y, int B, int H, int W, int C, float eps, void* stream);

/*
 * ConvNeXt block back half, fused: out = x + gamma * (W2 . GELU(W1 . y + b1) + b2)  (convNeXT/convnext.py:44-51: pwconv1, GELU,
 * pwconv2, layer scale, residual).  y, x, out dense [M][C]; w1 [4C][C], w2 [C][4C] in PyTorch layout.  The 4C-wide hidden
 * tensor never leaves registers.  Supported C: see kpf_convnext_mlp_supported(); other widths use two kpf_conv2d_f32 launches.
 * out may alias x.
 */
int kpf_convnext_mlp_f32(const float* y, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                         const float* gamma, float* out, long M, int C, void* stream);
int kpf_convnext_mlp_supported(int C);
/* The same block on the f16 matrix cores with split operands (see kpf_conv2d_f32): y is the split LayerNorm output
 * (kpf_dwconv7_ln_split_f32), w1 [4C][C] and w2 [C][4C] are split-packed and scaled by 1/w*_unscale (powers of two); inside each
 * 32-wide hidden block w2's columns are ordered k = 8g+j -> hidden 16*(j>>2) + 4g + (j&3), the order in which GEMM1's accumulator
 * registers become GEMM2's operand.  x and out are fp32. */
int kpf_convnext_mlp_split_f32(const float* y_split, const float* x, const float* w1_split, const float* b1, float w1_unscale,
                               const float* w2_split_perm, const float* b2, float w2_unscale, const float* gamma, float* out, long M,
                               int C, void* stream);
int kpf_convnext_mlp_split_supported(int C);
/* The same block on 16-bit storage (round 4; replaces the kpf_conv2d_h16 pair pwconv1 + GELU / pwconv2 + layer scale + residual of
 * convNeXT/convnext.py:44-51 where the hidden tensor's HBM round trip dominates — C = 128 / 256, the first two stages of ConvNeXt-B): y, x,
 * out [M][C] and w1 [4C][C] in the storage type `dtype` (KPF_DT_BF16 / KPF_DT_F16), fp32 biases and layer scale, fp32 accumulation and
 * arithmetic, one rounding of the result.  w2_chunks is pwconv2's weight [C][4C] repacked chunk-major, [4C/32][C][32], with the hidden index
 * inside each 32-block in the order k = 8g + j -> hidden 16*(j>>2) + 4g + (j&3) (the order of kpf_convnext_mlp_split_f32).  GELU is evaluated as
 * x * sigmoid(x (c1 + c3 x^2 + c5 x^4)), |error| <= 2.6e-5 absolute: below the rounding of a 16-bit result.  out may alias x. */
int kpf_convnext_mlp_h16(const void* y, const void* x, const void* w1, const float* b1, const void* w2_chunks, const float* b2,
                         const float* gamma, void* out, long M, int C, int dtype, void* stream);
int kpf_convnext_mlp_h16_supported(int C);

/*
 * Depthwise 7x7 + bias as a pure stencil that also emits LayerNorm statistics, and the LayerNorm from those statistics (round 4; together they
 * replace kpf_dwconv7_ln_h16 = convNeXT/convnext.py:41-44 on 16-bit storage for C % 64 == 0 and maps of at least 16 x 16):
 *   kpf_dwconv7_stats_h16   y = dwconv7(x) + b (un-normalised, storage type `dtype`), stats[pixel][C/64][2] = (mean, sum of centred squares) of
 *                           every 64-channel chunk of the fp32 result;  kpf_dwconv7_stats_floats = the floats `stats` needs.
 *   kpf_ln_apply_stats_h16  y <- (y - mean) * rstd * ln_w + ln_b in place, (mean, rstd) merged from the chunk statistics (Chan's update, fixed
 *                           order).  (The statistics are laid out for the following GEMM to consume them instead: out = rstd * (W'y - mean * s) + b'.)
 */
int kpf_dwconv7_stats_h16(const void* x, const float* w_dw, const float* b_dw, void* y, float* stats, int B, int H, int W, int C, int dtype,
                          void* stream);
int kpf_dwconv7_stats_supported(int H, int W, int C);
long kpf_dwconv7_stats_floats(int B, int H, int W, int C);
int kpf_ln_apply_stats_h16(void* y, const float* stats, const float* ln_w, const float* ln_b, long rows, int C, float eps, int dtype, void* stream);
/* mean_rstd[pixel] = (mean, 1 / sqrt(var + eps)) merged from the chunk statistics of kpf_dwconv7_stats_h16 exactly as kpf_ln_apply_stats_h16 merges them:
 * the operand statistics of a kpf_conv2d_h16 launch with KPF_PRO_LN (the nn.LayerNorm of convNeXT/convnext.py:42 folded into pwconv1, ABI 15). */
int kpf_ln_stats_merge(const float* stats, float* mean_rstd, long rows, int C, float eps, void* stream);

/*
 * LayerNorm over the channel dimension of `rows` pixels (biased variance, (x-u)/sqrt(var+eps)*w+b).
 * Replaces convNeXT/convnext.py:205-214 in both data formats (stem/downsample norms).  In-place allowed.
 */
int kpf_layernorm_f32(const float* x, const float* w, const float* b, float* y, long rows, int C, float eps, void* stream);

/* Same two ops writing their output in the split operand format of kpf_conv2d_f32 (C % 32 == 0): the LayerNorm output feeds only
 * pwconv1 / a downsample convolution, so it is split where it is produced. */
int kpf_dwconv7_ln_split_f32(const float* x, const float* w_dw, const float* b_dw, const float* ln_w, const float* ln_b, float* y,
                             int B, int H, int W, int C, float eps, void* stream);
int kpf_layernorm_split_f32(const float* x, const float* w, const float* b, float* y, long rows, int C, float eps, void* stream);

/*
 * Bilinear x2 upsampling, align_corners=False (nn.Upsample(scale_factor=2, mode='bilinear'),
 * convNeXT/resnetUnet.py:76-77): src dense NHWC [B][H][W][C] -> dst channel slice (ld, coff) of [B][2H][2W][*].
 */
int kpf_upsample2x_f32(const float* src, float* dst, int B, int H, int W, int C, int dst_ld, int dst_coff, void* stream);

/* NCHW [B][C][H][W] -> NHWC [B][H][W][Cpad] (channels >= C zero-filled).  Boundary repack of the inputs of
 * KPFusion.forward (model/model.py:395). */
int kpf_nchw_to_nhwc_f32(const float* src, float* dst, int B, int C, int H, int W, int Cpad, void* stream);

/* NHWC channel slice -> dense NCHW (boundary repack of returned tensors). */
int kpf_nhwc_to_nchw_f32(const float* src, float* dst, int B, int C, int H, int W, int src_ld, int src_coff, void* stream);

/* 3x3 stride-2 pad-1 max pooling on dense NHWC (model/resnet.py:169,236). */
int kpf_maxpool3x3s2_f32(const float* src, float* dst, int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Keypoint-fusion head (Block_KPFusion, model/model.py:287-351) — geometry, point-cloud and 21-token kernels.
 * J = 21 joints, feature maps F x F (P = F*F pixels), N points, C = 128 channels; all buffers dense fp32.
 * ------------------------------------------------------------------------------------------------------------ */

/* Inverse of B 3x3 crop matrices [B][3][3] -> Minv [B][3][3] in the operation order of the reference's torch.linalg.inv on the CPU
 * (dataloader/loader.py:781 -> ATen linalg_solve_ex on A^T -> LAPACK getrf/getrs), bit-identical to it, so that pixel positions and
 * the integer top-4 / ball-query decisions derived from them match the reference bit for bit.  fused = 1: the library's FMA code
 * path (Intel hosts), 0: its separately-rounded path (AMD hosts) — keypointfusion_amd/inv3x3.py::host_mode() tells which one the
 * host's torch.linalg.inv takes.  The geometry entry points below take this Minv (or one computed by torch.linalg.inv itself). */
int kpf_inv3x3_f32(const float* M, float* Minv, int B, int fused, void* stream);

/* Masked soft-argmax decode of the depth stream's offset maps + uvd->xyz (model/model.py:466-500 offset2joint_weight,
 * dataloader/loader.py:775-789 uvd_nl2xyznl_tensor).  offset NCHW [B][105][P]; depth [B][S][S] (nearest-downsampled to
 * F on the fly, model/model.py:471); center [B][3], Minv [B][3][3] (kpf_inv3x3_f32), cube [B][3], cam [B][4].
 * -> joint_uvd, joint_xyz [B][21][3]. */
int kpf_offset2joint_f32(const float* offset, const float* depth, const float* center, const float* Minv, const float* cube,
                         const float* cam, float* joint_uvd, float* joint_xyz, int B, int S, int F, float kernel,
                         int img_size, int flip, void* stream);

/* Per point the 4 nearest feature pixels, ascending squared distance, and inverse-distance weights
 * (dataloader/loader.py:936-967 img2pcl_index; replaces the B x N x P x 3 broadcast + ATen topk).
 * -> closeness [B][N][4] fp32, index [B][N][4] int32 (values in [0,P)), img_xyz [B][P][3] (pixel positions, may be NULL). */
int kpf_img2pcl_top4_f32(const float* pcl, const float* depth, const float* center, const float* Minv, const float* cube,
                         const float* cam, float* closeness, int* index, float* img_xyz, int B, int N, int S, int F,
                         int img_size, int flip, void* stream);

/* Point feature gather + pcl_joint2offset (model/model.py:295-309, 503-525): builds the operand rows of the point
 * embedding GEMMs: A1 [B*N][240] = [pf 128 | xyz 3 | pw 21 | unit offsets 63 | closeness 21 | 0 x4], A2 [B*N][128] = pf_rgb.
 * feat_* NHWC [B][P][128]; offset NCHW [B][105][P].  B * N % 4 == 0 (a workgroup takes four points; they may belong to two samples);
 * index values in [0, P). */
int kpf_point_assemble_f32(const float* feat_d, const float* feat_rgb, const float* offset, const float* pcl,
                           const float* joint_xyz, const float* closeness, const int* index, float* A1, float* A2, int B,
                           int N, int P, float kernel, void* stream);

/* attention = softmax_N(pw), joint_feat = attention @ X (model/model.py:319-320).  X [B*N][128];
 * -> JA [B*21][132] = [joint_feat 128 | joint xyz 3 | 0].  A1 is the [B*N][240] buffer of kpf_point_assemble_f32, of which only the pw columns 131..151
 * are read.  N % 4 == 0 and 4 <= N <= 2048 (7 N + 32 floats of LDS sit in front of an array that takes 16-byte stores; N > 1312 opts into > 64 KiB of LDS). */
int kpf_softmax_pool_f32(const float* A1, const float* X, const float* joint_xyz, float* JA, int B, int N, void* stream);

/* pointnet2_ops ball_query + group_points for the 3 DESA radii (model/model.py:158,171-178): points = cat(pcl, joints),
 * features = cat(X [B*N][128], JF [B*21][jf_ld]).  -> G [3][B*21*64][132] = [feat[idx]-feat_j | (xyz[idx]-xyz_j)/r | 0],
 * idx_out [3][B*21][64] int32 (may be NULL). */
int kpf_ball_group_f32(const float* pcl, const float* joint_xyz, const float* X, const float* JF, int jf_ld, float* G,
                       int* idx_out, int B, int N, float r0, float r1, float r2, void* stream);

/* max over groups of `group` consecutive rows (torch.max(dim=-1), model/model.py:198): in [rows*group][C] -> columns [out_coff, out_coff + C) of
 * out [rows][out_ld], out_coff + C <= out_ld.  Any C; C % 4 == 0, C <= 1024 with 16-byte aligned rows on both sides takes the float4 kernel (same bits). */
int kpf_group_max_f32(const float* in, float* out, long rows, int group, int C, int out_ld, int out_coff, void* stream);
/* The same grouping with the three radii CHANNEL-STACKED (ABI 16; the training step's grouped DESA launches): GF [B*21*64][3*128] grouped feature
 * differences, GX [B*21*64][3*4] offsets / radius (3 + a zero channel) — radius i in columns [128 i, 128 i + 128) / [4 i, 4 i + 4). */
int kpf_ball_group_stacked_f32(const float* pcl, const float* joint_xyz, const float* X, const float* JF, int jf_ld, float* GF, float* GX, int* idx_out,
                               int B, int N, float r0, float r1, float r2, void* stream);

/* Heat-map, geometry adjacency map, spatial attention, gate (model/model.py:334-338; util/generateFeature.py:584-600;
 * dataloader/loader.py:791-819).  SF [B*P][sf_ld] = feature part of atten_spatial (a GEMM), Wh [21][21] its heat-map part.
 * -> sw_out NCHW [B][21][P] (returned spatial weight), Gw [B][21][P] = gate * fc_spatial2joint_feature.weight. */
int kpf_heat_gam_gate_f32(const float* r3d, const float* img_xyz, const float* SF, int sf_ld, const float* Wh,
                          const float* bias, const float* weight_dis, const float* wfc, const float* center,
                          const float* Minv, const float* cube, const float* cam, float* sw_out, float* Gw, int B, int F,
                          int img_size, int flip, void* stream);

/* img_feat_j = Gw @ relu(feat) + b (model/model.py:340-344), optional relu((. + prev)/2).  -> out [B][21][128].
 * P % 32 == 0 (two pixel halves of 16-pixel MFMA blocks), Gw 16-byte aligned. */
int kpf_gate_reduce_f32(const float* Gw, const float* feat, const float* bfc, const float* prev, float* out, int B, int P,
                        void* stream);

/* KP_Interaction_TR (model/model.py:106-126): embed + 4 BERT layers + 3-vector heads on 21 tokens, one workgroup per
 * sample.  x [B*21][ldx] (Din used), W = packed weights (keypointfusion_amd/engine.py:pack_tr), -> h [B][21][128],
 * score [B][21][3]; score2 (may be NULL) receives a second copy with row stride score2_ld.
 * 0 < Din <= 208 (the [21][Din rounded up to 16] input tokens share the CU's 160 KiB of LDS with the rest of the stack; the model uses 128 and 131),
 * ldx >= Din; columns [Din, ldx) of x are not read. */
int kpf_tr_encoder_f32(const float* x, int ldx, int Din, const float* W, float* h, float* score, float* score2,
                       int score2_ld, int B, void* stream);
int kpf_tr_encoder_weight_floats(int Din);

/* The observable layer of updatedDecoder (model/transfusion_head.py:137-173 with cross_only): query/key [B][21][128]
 * -> out rows [B*21] with stride out_ld at column out_coff, out_coff + 128 <= out_ld. */
int kpf_xattn_layer_f32(const float* query, const float* key, const float* W, float* out, int out_ld, int out_coff, int B,
                        void* stream);
int kpf_xattn_weight_floats(void);

/* ---- stand-alone heads: named by the north star, not called by KPFusion.forward ---------------------- */

/* CBAM ChannelGate (model/cbam.py:26-57): scale[b][c] = sigmoid(mlp(avgpool(x)) + mlp(maxpool(x))), mlp = Linear(C,Cr) ReLU
 * Linear(Cr,C) with w1 [Cr][C], w2 [C][Cr] (nn.Linear layout).  x NHWC [B][HW][C]; workspace >= kpf_cbam_workspace_floats(). */
long kpf_cbam_workspace_floats(int B, int HW, int C);
int kpf_cbam_channel_gate_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                              float* workspace, float* scale, int B, int HW, int C, int Cr, void* stream);
/* CBAM SpatialGate value (model/cbam.py:65-81): comp [B][H][W][2] = (max_c, mean_c) of x*scale, then
 * sgate[b][y][x] = sigmoid(bn_scale * conv7x7_pad3(comp; w7 [2][7][7]) + bn_shift) (eval BatchNorm folded by the caller). */
int kpf_cbam_spatial_gate_f32(const float* x, const float* scale, const float* w7, float bn_scale, float bn_shift, float* comp,
                              float* sgate, int B, int H, int W, int C, void* stream);
/* out0 = (x*scale)*sgate, out1 = (x*scale)*(1-sgate) — the tuple SpatialGate.forward returns (model/cbam.py:82);
 * sgate == out1 == NULL: out0 = x*scale (CBAM(no_spatial=True), model/cbam.py:90-94). */
int kpf_cbam_apply_f32(const float* x, const float* scale, const float* sgate, float* out0, float* out1, int B, int HW, int C,
                       void* stream);

/* nn.MaxPool2d(2,2) on NHWC (model/hourglass.py:8,128) and nn.Upsample(scale_factor=2, nearest) fused with the hourglass
 * skip add `up1 + up2` (model/hourglass.py:138-149): out [B][2h][2w][C] = up1 + low[y/2][x/2]. */
int kpf_maxpool2x2_f32(const float* src, float* dst, int B, int H, int W, int C, void* stream);
int kpf_upnearest2x_add_f32(const float* low, const float* up1, float* out, int B, int h, int w, int C, void* stream);

/* mano_regHead tail (model/mano_head.py:212-225) + ManoLayer.forward (util/manopth/manopth/manolayer.py:106-273; use_pca=False,
 * axis-angle joints, right hand, no centring / translation): pose6d rows [B][ld6] (16 x 6D rotations), betas rows [B][ldb] (10)
 * -> verts [B][778][3] mm, joints [B][21][3] mm in OBMAN2MANO order, rotmat [B][16][3][3], pose_aa [B][48].
 * Model arrays: shapedirs_t [10][778*3], posedirs_t [135][778*3] (transposed blend-shape bases), v_template [778*3],
 * j_regressor [16][778], skin_weights [778][16], hands_mean [45]. */
int kpf_mano_forward_f32(const float* pose6d, int ld6, const float* betas, int ldb, const float* shapedirs_t,
                         const float* posedirs_t, const float* v_template, const float* j_regressor, const float* skin_weights,
                         const float* hands_mean, float* verts, float* joints, float* rotmat, float* pose_aa, int B, void* stream);

/* Backward of kpf_mano_forward_f32 (ABI 26).  Gradient inputs may each be NULL (= zero):
 * d_verts [B][778][3], d_joints [B][21][3] (head order, as the forward writes them),
 * d_rotmat [B][16][3][3], d_pose_aa [B][48].
 * Writes (overwrites, never accumulates) d_pose6d rows [B][ldd6] (first 96 columns)
 * and d_betas rows [B][lddb] (first 10); other columns untouched.
 * The forward is recomputed in LDS (no saved workspace); the gradient is torch autograd's of the same formulas (a clamped F.normalize and a selected
 * isnan pass no gradient), except at an exact identity rotation, where autograd gives NaN and this gives the derivative of the k = 2 branch the forward
 * takes there.  Fixed-order reductions: a sample's bits depend neither on B nor on its position nor on a replay. */
int kpf_mano_backward_f32(const float* pose6d, int ld6, const float* betas, int ldb,
    const float* shapedirs_t, const float* posedirs_t, const float* v_template, const float* j_regressor,
    const float* skin_weights, const float* hands_mean,
    const float* d_verts, const float* d_joints, const float* d_rotmat, const float* d_pose_aa,
    float* d_pose6d, int ldd6, float* d_betas, int lddb, int B, void* stream);

/* Fit the MANO layer to 21 target joints per sample (ABI 26): one workgroup per sample, all `iters` Adam iterations inside the one launch.
 * Per sample  L = (1 / sum w) sum_i w_i |J_map[i](theta, beta) + t - y_i|^2 + lambda_shape |beta|^2 + lambda_pose |theta[3:]|^2  in mm^2, minimised by
 * torch.optim.Adam's update (no weight decay, no amsgrad; moments zero at the start of every call; step k counts from 1 in the bias corrections;
 * step = lr m^ / (sqrt(v^) + eps)) with one learning rate each for pose, shape and translation.  init_trans != 0 (and iters > 0) first sets
 * t = sum w_i (y_i - J_i) / sum w.  pose_aa is the head's mano_pose_aa (hands_mean is added inside); rotmat[j] = rodrigues(pose_aa[j]).
 * status [B] bits: 1 sum w == 0; 2 a target with w > 0 is not finite — in both cases the state keeps its bits and the outputs evaluate it
 * (residual 0 for bit 1).  A target of weight 0 is selected out, never multiplied.  residual [B][2]: the mean weighted joint distance in mm at the
 * first state (after init_trans) and at the final one.  Same determinism as the backward. */
typedef struct kpf_mano_fit_cfg {
  int iters;                       /* 0 <= iters <= 1000; 0 only evaluates */
  float lr_pose, lr_shape, lr_trans, beta1, beta2, eps;
  float lambda_shape, lambda_pose; int init_trans;
  int joint_map[21];               /* target row i <-> head-order model joint joint_map[i]; a permutation */
} kpf_mano_fit_cfg;                /* HOST struct */
int kpf_mano_fit_f32(const float* target /*[B][21][3] mm*/, const float* weight /*[B][21] >= 0, or NULL = ones*/,
    const float* shapedirs_t, const float* posedirs_t, const float* v_template, const float* j_regressor,
    const float* skin_weights, const float* hands_mean, const kpf_mano_fit_cfg* cfg,
    float* pose_aa /*[B][48] in/out*/, float* betas /*[B][10] in/out*/, float* trans /*[B][3] mm in/out*/,
    float* verts /*[B][778][3] or NULL*/, float* joints /*[B][21][3], target order*/, float* rotmat /*[B][16][9] or NULL*/,
    float* residual /*[B][2]*/, int* status /*[B]*/, int B, void* stream);

/* The fit above with a vertex term (ABI 27).  Per sample, in mm^2:
 *   L = [sw > 0] (1/sw) sum_i w_i |J_map[i] + t - y_i|^2 + lambda_verts [sv > 0] (1/sv) sum_v u_v |V_v + t - c_v|^2
 *     + lambda_shape |beta|^2 + lambda_pose |theta[3:]|^2
 * with vert_target c [B][778][3] in mm, vert_weight u [B][778] >= 0, sw = sum w, sv = sum u.  A term whose weights sum to 0 contributes nothing; a
 * target under weight 0 (joint or vertex) is selected out, never multiplied.  vert_target == vert_weight == NULL: no vertex term, and every output is
 * bit for bit kpf_mano_fit_f32's (residual columns 0-1; columns 2-3 are 0).  target == NULL, or weights all 0, with a vertex term: a vertex-only fit.
 * init_trans uses the joints when sw > 0, otherwise t = sum u_v (c_v - V_v) / sv.  residual [B][4]: the mean weighted joint distance at the first
 * state (after init_trans) and at the final one, then the mean weighted vertex distance at the same two states; a term without weight reports 0.
 * status [B] bits: 1 BOTH weight sums are 0; 2 a joint or vertex target under a positive weight is not finite -- either way the state keeps its bits
 * and the outputs evaluate it.  Each iteration skins all 778 vertices; the vertex gradient and the translation's are reduced in a fixed order (wave
 * butterfly, then the four waves in order), no atomics: bits depend neither on B nor on the sample's position nor on a replay.  The output of
 * kpf_mano_assoc_f32 is this entry's vertex input; a ground-truth mesh is passed with u = 1. */
typedef struct kpf_mano_fit_mesh_cfg {
  int iters;                       /* as kpf_mano_fit_cfg, field for field ... */
  float lr_pose, lr_shape, lr_trans, beta1, beta2, eps;
  float lambda_shape, lambda_pose; int init_trans;
  int joint_map[21];
  float lambda_verts;              /* ... plus the vertex term's factor, >= 0 */
} kpf_mano_fit_mesh_cfg;           /* HOST struct */
int kpf_mano_fit_mesh_f32(const float* target /*[B][21][3] mm, or NULL*/, const float* weight /*[B][21] >= 0, or NULL = ones*/,
    const float* vert_target /*[B][778][3] mm, or NULL*/, const float* vert_weight /*[B][778] >= 0, or NULL; both or neither*/,
    const float* shapedirs_t, const float* posedirs_t, const float* v_template, const float* j_regressor,
    const float* skin_weights, const float* hands_mean, const kpf_mano_fit_mesh_cfg* cfg,
    float* pose_aa /*[B][48] in/out*/, float* betas /*[B][10] in/out*/, float* trans /*[B][3] mm in/out*/,
    float* verts /*[B][778][3] or NULL*/, float* joints /*[B][21][3], target order*/, float* rotmat /*[B][16][9] or NULL*/,
    float* residual /*[B][4]*/, int* status /*[B]*/, int B, void* stream);

/* The joint fit by damped Gauss-Newton (ABI 28): kpf_mano_fit_f32's objective, state, targets, weights, joint_map, outputs and status convention, one
 * workgroup per sample, every iteration inside the one launch, no atomics, fixed-order sums.  With p = (pose 0..47, betas 48..57, trans 58..60):
 *   r_i = sqrt(w_i / sw) (J_map[i](theta, beta) + t - y_i)   63 rows, mm; a row under weight 0 is selected out
 *   J = d r / d p (63 x 61),  Lambda = diag(0 x3, lambda_pose x45, lambda_shape x10, 0 x3)
 *   A = J^T J + Lambda + mu diag(J^T J) + nu I,  g = J^T r + Lambda p,  A delta = g by Cholesky,  p <- p - delta
 * with a fixed damping and no accept/reject step.  init_trans != 0 (and iters > 0) first sets t to the weighted mean offset, summed in double and rounded
 * once.  history [B][iters + 1] or NULL: the mean weighted joint distance before iteration 1 and after each iteration (first and last entry are
 * residual's).  jacobian [B][63][61] or NULL: the unweighted d (J_map[i] + t) / d p of the state on entry, in mm, rows in target order.
 * status bits 1 and 2 as kpf_mano_fit_f32; bit 4: a pivot of the factorisation was not > 0 or not finite -- the iteration stops, the state holds the
 * last completed iteration (after init_trans), the outputs evaluate it and the remaining history entries repeat its distance. */
typedef struct kpf_mano_fit_gn_cfg {
  int iters;                       /* 0 <= iters <= 64; 0 only evaluates */
  float mu, nu;                    /* Marquardt's relative damping and the absolute floor on the diagonal, both >= 0 */
  float lambda_shape, lambda_pose; int init_trans;
  int joint_map[21];               /* as kpf_mano_fit_cfg */
} kpf_mano_fit_gn_cfg;             /* HOST struct */
int kpf_mano_fit_gn_f32(const float* target /*[B][21][3] mm*/, const float* weight /*[B][21] >= 0, or NULL = ones*/,
    const float* shapedirs_t, const float* posedirs_t, const float* v_template, const float* j_regressor,
    const float* skin_weights, const float* hands_mean, const kpf_mano_fit_gn_cfg* cfg,
    float* pose_aa /*[B][48] in/out*/, float* betas /*[B][10] in/out*/, float* trans /*[B][3] mm in/out*/,
    float* verts /*[B][778][3] or NULL*/, float* joints /*[B][21][3], target order*/, float* rotmat /*[B][16][9] or NULL*/,
    float* residual /*[B][2]*/, int* status /*[B]*/, float* history /*[B][iters + 1] or NULL*/, float* jacobian /*[B][63][61] or NULL*/,
    int B, void* stream);

/* The Gauss-Newton fit with the vertex term (ABI 29): the iteration of kpf_mano_fit_gn_f32 over the 63 joint rows and 2334 vertex rows
 *   sqrt(lambda_verts u_v / sv) (V_v + t - c_v),  sv = sum u
 * with the targets, weights and nullability of kpf_mano_fit_mesh_f32 (vert_target and vert_weight both or neither; target == NULL with a vertex term is
 * a vertex-only fit; a call without either kind of target is refused, and so is vert_jacobian without a vertex term).  A row under weight 0 is selected out, never multiplied; a term whose weights sum to 0
 * contributes nothing.  N = J^T J over all rows, A = N + Lambda + mu diag(N) + nu I, g = J^T r + Lambda p, A delta = g by Cholesky, p <- p - delta; the
 * damping is fixed.  init_trans is kpf_mano_fit_mesh_f32's rule (the joints when sw > 0, otherwise the vertices; summed in double, rounded once).
 * status bits: 1 BOTH weight sums are 0; 2 a joint or vertex target under a positive weight is not finite (either: the state keeps its bits, the outputs
 * evaluate it); 4 a pivot is not > 0 or not finite (the state holds the last completed iteration, the history repeats).  residual [B][4] as
 * kpf_mano_fit_mesh_f32.  history [B][iters + 1][2] or NULL: the mean weighted joint and vertex distance before iteration 1 and after each iteration.
 * jacobian [B][63][61] or NULL as kpf_mano_fit_gn_f32; vert_jacobian [B][2334][61] or NULL (vertex term only): the unweighted d (V_v + t) / d p of the
 * state on entry, mm, row v * 3 + d.  Without a vertex term the launch is kpf_mano_fit_gn_f32's kernel: state, joints, verts, rotmat, status,
 * residual[:, :2] and history[..., 0] are its bits, the vertex distances are 0.  With it: one 256-thread workgroup per hand, every iteration inside the
 * launch, J^T J and J^T r accumulated on v_mfma_f32_16x16x4_f32 in a fixed order, no atomics: bits depend neither on B nor on position nor on a replay. */
typedef struct kpf_mano_fit_mesh_gn_cfg {
  int iters;                       /* as kpf_mano_fit_gn_cfg, field for field ... */
  float mu, nu;
  float lambda_shape, lambda_pose; int init_trans;
  int joint_map[21];
  float lambda_verts;              /* ... plus the vertex term's factor, >= 0 */
} kpf_mano_fit_mesh_gn_cfg;        /* HOST struct */
int kpf_mano_fit_mesh_gn_f32(const float* target /*[B][21][3] mm, or NULL*/, const float* weight /*[B][21] >= 0, or NULL = ones*/,
    const float* vert_target /*[B][778][3] mm, or NULL*/, const float* vert_weight /*[B][778] >= 0, or NULL; both or neither*/,
    const float* shapedirs_t, const float* posedirs_t, const float* v_template, const float* j_regressor,
    const float* skin_weights, const float* hands_mean, const kpf_mano_fit_mesh_gn_cfg* cfg,
    float* pose_aa /*[B][48] in/out*/, float* betas /*[B][10] in/out*/, float* trans /*[B][3] mm in/out*/,
    float* verts /*[B][778][3] or NULL*/, float* joints /*[B][21][3], target order*/, float* rotmat /*[B][16][9] or NULL*/,
    float* residual /*[B][4]*/, int* status /*[B]*/, float* history /*[B][iters + 1][2] or NULL*/, float* jacobian /*[B][63][61] or NULL*/,
    float* vert_jacobian /*[B][2334][61] or NULL*/, int B, void* stream);

/* Depth points -> per-vertex targets (ABI 27), one workgroup per hand.  points [B][N][3] in camera-space mm (the frame of the tracker's cam_mm),
 * 1 <= N <= 4096 (any other N is refused and nothing is written); point_weight [B][N] or NULL = ones; verts [B][778][3] (a fit's verts);
 * max_dist2: squared gate in mm^2.  idx [B][N]: the nearest vertex or -1; vert_target / vert_weight: per vertex the weighted centroid and the summed
 * weight of the points assigned to it (0 and 0 where there are none); stats [B][2]: the number of matched points and their mean distance to their
 * vertex in mm.  Arithmetic, every operation individually rounded (no fma): dx = p.x - v.x, ...; d2 = (dx*dx + dy*dy) + dz*dz; the argmin runs over
 * v = 0..777 ascending with a strict < (from d2 = +inf at v = 0); a point is matched iff its weight > 0, its coordinates are finite and
 * d2 <= max_dist2; per vertex W = sum w_n and S = sum w_n * p_n over its points in ascending n, c = S / W; stats[1] = (sum over matched n, ascending,
 * of sqrt(d2_n)) / count.  A numpy-fp32 restatement gives the same bits. */
int kpf_mano_assoc_f32(const float* points, const float* point_weight, const float* verts, float max_dist2,
    int* idx, float* vert_target, float* vert_weight, float* stats, int B, int N, void* stream);

/* Area-weighted vertex normals (ABI 30), one workgroup per hand, no atomics.  verts [B][778][3]; faces [F][3] int (the model's th_faces), 1 <= F <= 2048;
 * sign +1 or -1 (-1: a mirrored hand or the other winding).  Anything else is refused and nothing is written.  A face with an index outside 0..777 is
 * skipped.  Per face e1 = v1 - v0, e2 = v2 - v0, fn = e1 x e2 (fn.x = e1.y*e2.z - e1.z*e2.y, ...; unnormalised); per vertex S = the sum of fn over the
 * faces in ascending order, once for each corner of the face that is the vertex; len = sqrt((S.x*S.x + S.y*S.y) + S.z*S.z); normals [B][778][3] =
 * sign * (S / len) if len > 0 and finite, else (0, 0, 0) -- a vertex in no face, a cancelling fan, a NaN vertex's neighbourhood.  Every operation is
 * individually rounded (no fma): a numpy-fp32 restatement gives the same bits. */
int kpf_mano_normals_f32(const float* verts /*[B][778][3] mm*/, const int* faces /*[F][3]*/, int F, float sign /*+1 or -1*/,
    float* normals /*[B][778][3]*/, int B, void* stream);

/* kpf_mano_assoc_f32 over the vertices that face the camera (ABI 30): its N limits, weights, gate, argmin rule, centroid rule and rounding.  The camera is
 * the origin of the frame.  normals [B][778][3] (kpf_mano_normals_f32's); 0 <= facing_min < 1.  visible [B][778]: 1 iff n_v is finite and not all-zero and
 * (n.x*V.x + n.y*V.y) + n.z*V.z < -(facing_min * sqrt((V.x*V.x + V.y*V.y) + V.z*V.z)).  The argmin runs over the visible vertices only (ascending,
 * strict <); with no visible vertex every idx is -1.  stats [B][4]: the matched points, their mean distance to their vertex, the mean of
 * |(n_i.x*d.x + n_i.y*d.y) + n_i.z*d.z| with d = p - V_i over the matched points in ascending order, the number of visible vertices. */
int kpf_mano_assoc_vis_f32(const float* points, const float* point_weight, const float* verts, const float* normals /*[B][778][3]*/,
    float max_dist2, float facing_min /*0 <= . < 1*/, int* idx, float* vert_target, float* vert_weight,
    int* visible /*[B][778]*/, float* stats /*[B][4]*/, int B, int N, void* stream);

/* kpf_mano_assoc_vis_f32 with a vertex mask (ABI 31): vert_mask [B][778] int, or NULL = none.  A vertex is a candidate iff it passes the facing rule AND
 * vert_mask[v] != 0; visible and stats[3] report the combination.  The same kernel: with NULL or a mask of ones every output is
 * kpf_mano_assoc_vis_f32's bits.  The mask the fit uses is 1 - occluded of kpf_mano_raster_f32. */
int kpf_mano_assoc_vis_mask_f32(const float* points, const float* point_weight, const float* verts, const float* normals,
    const int* vert_mask /*[B][778] or NULL*/, float max_dist2, float facing_min, int* idx, float* vert_target, float* vert_weight,
    int* visible, float* stats, int B, int N, void* stream);

/* z-buffer render of the mesh into a crop's pixel grid (ABI 31), one workgroup per hand, the buffer in LDS.  verts [B][778][3] mm in the camera frame
 * of the depth points; faces [F][3] int, 1 <= F <= 2048; cam [B][4] = fx, fy, u0, v0; M [B][2][3], the affine map from frame pixels to crop
 * coordinates (the top two rows of the preprocessing's M), or NULL = the identity; 1 <= H, W and H * W <= 16384; margin in mm, finite and >= 0;
 * depth_obs [B][H][W] mm or NULL.  Anything else is refused before the launch and nothing is written.
 *   Per vertex U = (x*fx)/z + u0, V = (y*fy)/z + v0, sx = ((m00*U + m01*V) + m02) - 0.5, sy = ((m10*U + m11*V) + m12) - 0.5, iz = 1/z.  The -0.5: the
 * preprocessing back-projects crop pixel (c, r) from (c + 0.5, r + 0.5), so pixel (c, r) is sampled at sx = c, sy = r.
 *   Per face (i0, i1, i2): skipped if an index is outside 0..777, two indices are equal, or a vertex is not finite or has z <= 0 -- there is NO
 * near-plane clipping, a face that crosses z = 0 is dropped whole.  The edge function of a directed edge a -> b at p is evaluated from the lower index,
 * e = (sx[hi]-sx[lo])*(py-sy[lo]) - (sy[hi]-sy[lo])*(px-sx[lo]), and negated if a > b.  area = edge(i0 -> i1) at vertex i2; skipped if 0 or not finite.
 * w0, w1, w2 = edge(i1 -> i2), edge(i2 -> i0), edge(i0 -> i1) at the pixel; inside iff all three sign(area)*w_i >= 0 (two-sided).  The pixels are
 * ceil(min) .. floor(max) per axis, clamped to the window in float.
 *   Per inside pixel sum = (w0 + w1) + w2, izp = ((w0/sum)*iz0 + (w1/sum)*iz1) + (w2/sum)*iz2, d = 1/izp; a candidate iff d is finite and > 0.  The
 * smallest d wins the pixel, among equal d the lowest face index (an integer min on (bits(d) << 32) | face: no dependence on arrival order).
 *   depth [B][H][W] mm, 0 where nothing covers the pixel; face [B][H][W], -1 there.  occluded [B][778] = 1 iff the vertex is finite with z > 0, its
 * nearest pixel (floor(sx + 0.5), floor(sy + 0.5)) is inside the window, that pixel is covered and depth[pixel] < z - margin.  stats [B][4]: covered
 * pixels; observed pixels (depth_obs finite and > 0); pixels that are both; the mean of |d - d_obs| over those, summed per row in ascending column
 * order and then over the rows in ascending order (0 without any).  Without depth_obs entries 1..3 are 0.  Every operation is individually rounded
 * (no fma): a numpy-fp32 restatement gives the same bits. */
int kpf_mano_raster_f32(const float* verts, const int* faces, int F, const float* cam, const float* M /*or NULL*/, int H, int W, float margin,
    const float* depth_obs /*or NULL*/, float* depth, int* face, int* occluded, float* stats, int B, void* stream);

/* The silhouette of an observed depth crop (ABI 33), once per frame: for every pixel the nearest observed pixel, and the nearest observed depth around
 * it.  One workgroup per hand, integers and exact minima only.  depth_obs [B][H][W] mm, 1 <= H, W and H * W <= 16384; a pixel is OBSERVED iff its depth
 * is finite and > 0 (kpf_mano_raster_f32's rule).  Anything else is refused before the launch and nothing is written.
 *   dist2 [B][H][W] = the smallest (r - r')^2 + (c - c')^2 over the observed pixels (r', c') of the hand; nearest [B][H][W] = r' * W + c' of the observed
 * pixel with the smallest (dist2, r', c') in lexicographic order -- among equally near pixels the lowest linear index.  Both are -1 everywhere for a hand
 * with no observed pixel.  front [B][H][W] = the minimum of the observed depths among the pixels (r + i, c + j), i, j in -1..1, that lie in the window; 0
 * where none of them is observed.  count [B] = the number of observed pixels.  No output may overlap depth_obs. */
int kpf_depth_silhouette_f32(const float* depth_obs /*[B][H][W] mm*/, int H, int W, int* nearest /*[B][H][W]*/, int* dist2 /*[B][H][W]*/,
    float* front /*[B][H][W]*/, int* count /*[B]*/, int B, void* stream);

/* The free-space term of the cloud fit (ABI 33), once per round: a vertex that projects outside the observed silhouette is pulled to it, a vertex in
 * front of the observed surface is pushed back along its ray, and either replaces that vertex's entry in the vertex targets of the mesh fit.  One
 * workgroup per hand.  verts, cam, M (or NULL = the identity), H, W as kpf_mano_raster_f32; nearest, dist2, front [B][H][W]: kpf_depth_silhouette_f32's;
 * slack2 >= 0; margin in mm, > 0 or +inf (+inf: the in-front rule is off); step in mm, > 0 or +inf (+inf: no clamp); lambda_free finite and >= 0;
 * vert_target_in [B][778][3] and vert_weight_in [B][778] (both or neither: kpf_mano_assoc_*'s outputs), vert_normal_in [B][778][3] or NULL
 * (kpf_mano_normals_f32's).  Anything else is refused before the launch and nothing is written.
 *   Per vertex (x, y, z): U, V, sx, sy are kpf_mano_raster_f32's expressions; ok iff x, y, z are finite, z > 0 and neither sx nor sy is NaN.  The pixel
 * is (c, r) = (floor(sx + 0.5), floor(sy + 0.5)), each clamped to [0, W - 1], [0, H - 1] in float before the conversion: a vertex OUTSIDE the window is
 * judged at the nearest window pixel.  d2 = dist2[r][c], f = front[r][c].  m = M or ((1, 0, 0), (0, 1, 0)); det = m00*m11 - m01*m10; a hand whose det
 * is 0 or not finite has no vertex of kind 1 or 2.
 *   kind 1 (outside the silhouette) iff ok and d2 > slack2 (so d2 >= 0): the target keeps z and sits at the centre of pixel n = nearest[r][c],
 * c* = n % W, r* = n / W:  a = ((float)c* + 0.5) - m02, b = ((float)r* + 0.5) - m12, u = (m11*a - m01*b) / det, v = (m00*b - m10*a) / det,
 * t = (((u - u0) / fx) * z, ((v - v0) / fy) * z, z).
 *   kind 2 (in front of the observed surface) iff ok and d2 == 0 and f > 0 and z < f - margin: zt = f - margin, s = zt / z, t = (x*s, y*s, zt).
 *   kind 0: everything else.
 *   The clamp: d = t - (x, y, z), len = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z); kind becomes 0 if len is 0 or not finite; if len > step then
 * q = step / len and t = (x + d.x*q, y + d.y*q, z + d.z*q).
 *   kind 0 copies vert_target_in, vert_weight_in, vert_normal_in of the vertex bit for bit (zeros for an input that is NULL); kind 1 and 2 write t,
 * lambda_free (on the scale where one depth point weighs 1) and d / len: the vertex's matches in the cloud are dropped for the round, and the
 * point-to-plane row of kpf_mano_fit_mesh_gn_plane_f32 sees the whole pull.  kind [B][778].  stats [B][4]: the vertices of kind 1, the mean of
 * sqrt((float)d2) over them, the vertices of kind 2, the mean of f - z over them (0 without any).  Each sum: thread t of 256 adds its vertices t,
 * t + 256, ... in ascending order onto +0, a 64-lane butterfly (offsets 32, 16, ... 1) per wave, then ((w0 + w1) + w2) + w3.  Every operation is
 * individually rounded (no fma): a numpy-fp32 restatement gives the same bits. */
int kpf_mano_free_space_f32(const float* verts, const float* cam, const float* M /*or NULL*/, int H, int W, const int* nearest, const int* dist2,
    const float* front, int slack2, float margin, float step, float lambda_free, const float* vert_target_in /*or NULL*/,
    const float* vert_weight_in /*or NULL*/, const float* vert_normal_in /*or NULL*/, float* vert_target, float* vert_weight, float* vert_normal,
    int* kind /*[B][778]*/, float* stats /*[B][4]*/, int B, void* stream);

/* kpf_mano_fit_mesh_gn_f32 with a point-to-plane vertex term (ABI 30).  vert_normal [B][778][3], fixed for the launch, or NULL: then this is
 * kpf_mano_fit_mesh_gn_f32, the same kernel and bits.  With normals a vertex term is required, and each vertex contributes ONE row
 *   sqrt(lambda_verts u_v / sv) n_v^T (V_v + t - c_v),  Jacobian n_v^T d (V_v + t) / d p
 * (against the association's centroid: sum w_n (n.(V - p_n))^2 and W (n.(V - c))^2 have the same gradient).  Joint rows, Lambda, damping, solve,
 * init_trans and status bits 1, 2, 4 are kpf_mano_fit_mesh_gn_f32's; bit 2 is also set by a non-finite normal under a positive weight; a zero normal
 * under a positive weight gives a zero row and still counts in sv.  Column 1 of history and columns 2, 3 of residual report the mean weighted
 * |n_v . (V_v + t - c_v)|.  jacobian / vert_jacobian are unchanged (unweighted, unprojected). */
int kpf_mano_fit_mesh_gn_plane_f32(const float* target, const float* weight, const float* vert_target, const float* vert_weight,
    const float* vert_normal /*[B][778][3] or NULL*/, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
    const float* j_regressor, const float* skin_weights, const float* hands_mean, const kpf_mano_fit_mesh_gn_cfg* cfg,
    float* pose_aa, float* betas, float* trans, float* verts, float* joints, float* rotmat, float* residual /*[B][4]*/, int* status,
    float* history, float* jacobian, float* vert_jacobian, int B, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Reduced-precision path (BASELINE configs[2] bf16, configs[4] fp16): same operators on 16-bit NHWC activations.  `dtype` is
 * KPF_DT_BF16 or KPF_DT_F16; LayerNorm / bias / layer-scale parameters and the depthwise taps stay fp32.
 * ------------------------------------------------------------------------------------------------------------ */

/* kpf_conv2d_f32 on 16-bit operands: in / w / res / out are `dtype` (w rows [N][Kp], Kp % 64 == 0, Cin % 8 == 0), bias / gamma /
 * prologue scale+shift fp32, fp32 accumulation on v_mfma_f32_16x16x32_{bf16,f16}.  With KPF_OUT_NCHW the output is fp32 NCHW (the
 * heads).  The split-operand flags do not apply. */
int kpf_conv2d_h16(const kpf_conv_desc* desc, const void* in, const void* w, const float* bias, const float* pro_scale,
                   const float* pro_shift, const float* gamma, const void* res, void* out, int dtype, void* stream);
/* 1 when kpf_conv2d_h16 runs `d` on the eight-phase 256 x 256 kernel (gemm16_8ph_kernel: dense 1x1, K % 128 == 0, N % 256 == 0, at least 224 tiles), 0 when
 * on igemm_h16_kernel — for callers that label per-kernel measurements (bench.py's roofline); has_prologue: pro_scale != NULL. */
int kpf_conv2d_h16_uses_8ph(const kpf_conv_desc* d, int has_prologue);
/* 1 when kpf_conv2d_h16 accepts `d` with KPF_PRO_LN (ABI 15): GELU epilogue on a dense 1x1 layer with Cin == Kp, Kp % 128 == 0, N % 256 == 0 — a rule over
 * the layer's shape, never over its batch (the arithmetic of a sample must not depend on the size of its batch). */
int kpf_conv2d_h16_ln_fold_supported(const kpf_conv_desc* d);

/* kpf_dwconv7_ln_f32 with 16-bit activations in and out (fp32 taps, fp32 accumulation and LayerNorm statistics). */
int kpf_dwconv7_ln_h16(const void* x, const float* w_dw, const float* b_dw, const float* ln_w, const float* ln_b, void* y, int B,
                       int H, int W, int C, float eps, int dtype, void* stream);

/* LayerNorm over C: x_dtype -> y_dtype, either fp32 -> 16-bit (behind the fp32 stem convolution) or 16-bit -> the same type. */
int kpf_layernorm_h16(const void* x, int x_dtype, const float* w, const float* b, void* y, int y_dtype, long rows, int C, float eps,
                      void* stream);

/* kpf_upsample2x_f32 on 16-bit activations (dst_ld / dst_coff in elements). */
int kpf_upsample2x_h16(const void* src, void* dst, int B, int H, int W, int C, int dst_ld, int dst_coff, int dtype, void* stream);

/* 16-bit NHWC channel slice -> dense fp32 [rows][C] (feature maps handed to the fp32 fusion head / module boundary). */
int kpf_cast_h16_f32(const void* src, int dtype, float* dst, long rows, int C, int src_ld, int src_coff, void* stream);

/* dense fp32 [n] -> 16-bit (behind the fp32 stem + max-pool of the ResNet backbones); n % 4 == 0. */
int kpf_cast_f32_h16(const float* src, void* dst, int dtype, long n, void* stream);

/*
 * Training: weight and bias gradients of nn.Conv2d / nn.Linear — what autograd's convolution_backward /
 * addmm_backward compute for the layers of kpf_conv2d_f32 when the reference trains (train.py:198-232).
 *     dw[n][c][ky][kx] = sum_{b,oy,ox} dy[b][oy][ox][n] * x[b][oy*sh+ky-ph][ox*sw+kx-pw][c]      (OIHW, PyTorch's layout)
 *     db[n]            = sum_{b,oy,ox} dy[b][oy][ox][n]                                           (db may be NULL)
 * dy: NHWC [B][OH][OW] with pixel stride ldy (N channels used), x: NHWC [B][H][W] with pixel stride ldx (Cin channels used);
 * Cin, N, ldx, ldy multiples of 4, 16-byte aligned pointers.  Split over the pixel range with a fixed-order (run-to-run deterministic)
 * reduction through `ws` (>= groups * kpf_conv2d_wgrad_ws_floats(B*OH*OW, N, KH*KW*Cin) floats).
 * dtype (both operands): KPF_DT_F32 — fp32 on v_mfma_f32_16x16x4_f32; KPF_DT_BF16 / _F16 (mixed-precision training; Cin, N, ldx, ldy % 8 == 0) —
 *   16-bit storage, products and sums are the fp32 ones (the master weight's gradient is not rounded); KPF_DT_F32_MMA_BF16 / _F16 — see their definition.
 * groups (1..64; ABI 13; the data-parallel twin of kpf_conv_desc::groups): G channel-stacked weight gradients in one launch.  Group g multiplies
 *   dy[.., g*N + n] (pixel stride ldy >= G*N) with x[.., g*Cin + c] (pixel stride ldx >= G*Cin) and writes dw[g][N][Cin][KH][KW], db[g][N].  Same kernels as
 *   G separate calls on the channel slices; fp32 operands also keep their split and summation order (bit-identical results), 16-bit operands split the
 *   pixel range for 1/G of the chip each (same sums, another order).
 * cin_valid / n_valid (0 = all of Cin / N): the operands carry zero channels up to whole channel groups (the 3-, 105-, 131-, 149-wide layers of the fusion
 *   head, model/model.py:99-104, 254-262) and dw [n_valid][cin_valid][KH][KW], db [n_valid] are written without them.
 * reduce == NULL: the call launches its own reduce and dw / db are written when it returns (in stream order).
 * reduce != NULL (ABI 17; `loss.backward()` of train.py:262 issues ~100 weight-gradient GEMMs whose partial sums each needed a 5-us reduce launch): the
 *   call launches the split GEMM only and describes the pending reduce in *reduce (kind < 0: the call wrote dw itself, nothing is pending).  Until
 *   kpf_wgrad_reduce_multi has run on the same stream, dw / db are UNWRITTEN and ws belongs to the pending reduce.  kpf_wgrad_reduce_multi sums
 *   in the order the per-call reduce does: the gradients have the same bits either way.
 */
#define KPF_WGRAD_REDUCE_BATCH 24
typedef struct kpf_wgrad_reduce_desc {
  const float* part;   /* [S][N*K] partial tiles ([S][49][C] for the depthwise form) */
  const float* dbpart; /* [S][N] or NULL */
  float* dw;
  float* db;
  long g_ws;           /* floats between the workspaces of consecutive channel groups */
  int S, N, K, Cin, KHW, nkb, ndb, groups, Cin_out, N_out;
  int kind;            /* 0 convolution / Linear, 1 depthwise 7x7 (N = C), < 0 nothing pending */
  int first_block;     /* filled by kpf_wgrad_reduce_multi */
} kpf_wgrad_reduce_desc;
long kpf_conv2d_wgrad_ws_floats(long M, int N, int K);
int kpf_conv2d_wgrad(const void* dy, const void* x, int dtype, float* dw, float* db, float* ws, long ws_floats, int groups, int B, int H, int W, int Cin,
                     int ldx, int OH, int OW, int N, int ldy, int KH, int KW, int sh, int sw, int ph, int pw, int cin_valid, int n_valid,
                     kpf_wgrad_reduce_desc* reduce /* nullable */, void* stream);
int kpf_wgrad_reduce_multi(const kpf_wgrad_reduce_desc* descs, int n, void* stream);
/* Which kernel kpf_conv2d_wgrad gives a call, and a switch to pin it (ABI 22; tests and tuning: the tile shapes otherwise follow from cost models over M, N, K).
 * kpf_conv2d_wgrad_plan asks the dispatcher's own selection function — with what it decides from: dtype (any of kpf_conv2d_wgrad's), groups, M = B*OH*OW, N,
 * K = KH*KW*Cin, is_1x1 (KH == KW == 1), trimmed (cin_valid < Cin or n_valid < N) — and makes no device call.  family: _F32 wgrad_f32_kernel<vn, vk> (output
 * tile 32 vn x 32 vk; also the widening form of 16-bit operands, KPF_WGRAD_H16_WIDEN=1), _R16 wgrad_r16_kernel (KPF_DT_F32_MMA_* on the 64 x 64 tile; on any other
 * tile the fp32 products: _F32), _DIRECT the 64 x 64 fp32 tile unsplit over the <= 128 rows of a 1x1, _H16S / _H16 the 64- / 128-tile kernels of 16-bit operands.
 * S splits of sps stages each (32 pixels a stage, 128 in _H16S); writes_dw: an unsplit untrimmed 1x1 — the kernel writes dw / db itself, ws is not touched and a
 * descriptor comes back with kind < 0; ws_floats: what ONE group needs (kpf_conv2d_wgrad accepts groups * ws_floats; kpf_conv2d_wgrad_ws_floats is the bound
 * over every dtype and kernel size, forced tile included).
 * kpf_conv2d_wgrad_force_form: process-wide, 0 = the cost models (the default).  KPF_WGRAD_FORM_F32_* pins the tile of every call the fp32-MFMA kernels take and
 * switches the _DIRECT shortcut off; KPF_WGRAD_FORM_H16S / _H16 pins the kernel of every call with 16-bit operands, over the few-pixels rule and KPF_WG16_FORM
 * (_H16 with the split of its own plan).  A value of the other family leaves a call to the rules.  Not meant to change while calls are being issued. */
#define KPF_WGRAD_FAMILY_F32 0
#define KPF_WGRAD_FAMILY_R16 1
#define KPF_WGRAD_FAMILY_DIRECT 2
#define KPF_WGRAD_FAMILY_H16S 3
#define KPF_WGRAD_FAMILY_H16 4
#define KPF_WGRAD_FORM_F32_2x2 1 /* (vn, vk) = (2, 2): 64 x 64 */
#define KPF_WGRAD_FORM_F32_2x4 2 /* 64 x 128 */
#define KPF_WGRAD_FORM_F32_4x2 3 /* 128 x 64 */
#define KPF_WGRAD_FORM_F32_4x4 4 /* 128 x 128 */
#define KPF_WGRAD_FORM_H16S 5
#define KPF_WGRAD_FORM_H16 6
typedef struct kpf_wgrad_plan {
  int family, vn, vk, tiles_n, tiles_k, S, sps, writes_dw;
  long ws_floats;
} kpf_wgrad_plan;
int kpf_conv2d_wgrad_plan(int dtype, int groups, long M, int N, int K, int is_1x1, int trimmed, kpf_wgrad_plan* out);
int kpf_conv2d_wgrad_force_form(int form);

/* Row pad / column-slice copy / type change in one launch, and the pose tokens of a fusion block at their padded width (csrc/kpf_train.hip). */
int kpf_pad_rows(const void* src, int src_dtype, void* dst, int dst_dtype, long rows, int C, int src_ld, int Cp, void* stream);
/* Training (ABI 17): channel-stacked maps of G <= 4 paired networks <-> one dense fp32 map per network (train_graph.TrainGraph._forward: the seam between the
 * paired backbones and the fusion head).  src [rows][ld] (KPF_DT_*), group g's C channels at column g * gs; dst [G][rows][C] fp32.  kpf_restack_rows is the
 * gradient: grads[g] fp32 [rows][C] or NULL (zero) -> dst [rows][ld] of dst_dtype, every column (also the pad columns) written once. */
int kpf_unstack_rows(const void* src, int src_dtype, float* dst, long rows, int G, int C, int ld, int gs, int hw, void* stream);
int kpf_restack_rows(const float* const* grads, void* dst, int dst_dtype, long rows, int G, int C, int ld, int gs, int hw, void* stream);
/* hw > 0 (rows % hw == 0): the dense maps are NCHW — dst [G][rows / hw][C][hw], grads[g] [rows / hw][C][hw] — the layout the reference returns its offset maps
 * in (model/model.py:425) and the decode / the loss read; hw == 0: rows of C as above. */
int kpf_pose_tokens_f32(const float* pw, const float* joint, const float* pcl, float* out, int B, int N, int J, int ld, float kernel, void* stream);
/* out = relu(scale * (a + b + c)) (b, c nullable; fp32, n % 4 == 0) and d = out > 0 ? scale * dy : 0 — the gradient of every addend (ABI 13;
 * model/model.py:190, 417-422). */
int kpf_add_relu_forward(const float* a, const float* b, const float* c, float* out, long n, float scale, void* stream);
int kpf_add_relu_backward(const float* dy, const float* out, float* dx, long n, float scale, void* stream);
/* The gate of a fusion block around its two maps (ABI 13; model/model.py:334-341): sw = sigmoid(logits) (returned to the loss), gw = (sigmoid(weight_dis) * gam +
 * (1 - sigmoid(weight_dis)) * sw) * w_fc[p].  logits [B*P][J] (the rows of the atten_spatial GEMM), gam / sw / gw [B][J][P], weight_dis [1], w_fc [P].
 * backward: d_sw nullable; ws >= B*J floats; parameter gradients summed in a fixed order. */
int kpf_gate_mix_forward(const float* logits, const float* gam, const float* weight_dis, const float* w_fc, float* sw, float* gw, int B, int J, int P, void* stream);
int kpf_gate_mix_backward(const float* sw, const float* gam, const float* weight_dis, const float* w_fc, const float* d_sw, const float* d_gw, float* d_gam,
                          float* d_logits, float* d_w_fc, float* d_weight_dis, float* ws, int B, int J, int P, void* stream);
/* Depthwise 7x7 (pad 3) + bias alone, y = dwconv(x): the ConvNeXt block's first op with its output kept for the LayerNorm backward,
 * and its data gradient (dx = the same convolution of dy with w_dw's taps mirrored, zero bias).  w_dw [49][C], x != y. */
int kpf_dwconv7_f32(const float* x, const float* w_dw, const float* b_dw, float* y, int B, int H, int W, int C, void* stream);
/* the same + addend (y's shape) on the output: the data gradient of a ConvNeXt block with the skip path's gradient folded in */
int kpf_dwconv7_add_f32(const float* x, const float* w_dw, const float* b_dw, const float* addend, float* y, int B, int H, int W, int C, void* stream);
/* The weight gradient of the ConvNeXt block's depthwise 7x7 (pad 3): dw [C][7][7] (= PyTorch's [C][1][7][7]), db [C] or NULL; dy, x dense NHWC
 * [B][H][W][C], C % 4 == 0; ws >= kpf_dwconv7_wgrad_ws_floats(B, H, C) floats.  reduce (nullable): as kpf_conv2d_wgrad's — NULL reduces at once,
 * otherwise dw / db stay UNWRITTEN until kpf_wgrad_reduce_multi. */
long kpf_dwconv7_wgrad_ws_floats(int B, int H, int C);
int kpf_dwconv7_wgrad(const float* dy, const float* x, float* dw, float* db, float* ws, long ws_floats, int B, int H, int W, int C,
                      kpf_wgrad_reduce_desc* reduce /* nullable */, void* stream);
/* Which kernel the depthwise 7x7 entry points give a call (ABI 24; tests and tuning).  kpf_dwconv7_plan asks the launchers' own selection functions and makes no
 * device call.  op: _LN kpf_dwconv7_ln_f32 / _split_f32 / _h16 (dtype KPF_DT_F32 | _BF16 | _F16; split != 0: the split output, fp32 storage and C % 32 == 0 only),
 * _FWD kpf_dwconv7_f32 / _add_f32, _WGRAD kpf_dwconv7_wgrad (both fp32; split must be 0).  A shape the entry point refuses is refused here.  The tuning switches
 * of the environment (KPF_DW_TILE, KPF_DW_UNFUSED, KPF_DW_WIDE, KPF_DW_WIDE_ROWS, KPF_DW_PX; KPF_DW7_PX, KPF_DW7_ROWS, KPF_DW7_MIN_BLOCKS; KPF_DW7_WGRAD_LDS,
 * KPF_DW7_TARGET, KPF_DW7_MINROWS) are defaults of the selection, read once per process: the answer is the choice under them.
 *   family   _TILE   dwconv7_ln_tile_kernel<nchk, px>: LDS halo tiles of `rows` x 4 px pixels, C = 32 nchk
 *            _WAVE   dwconv7_ln_wave_kernel<lg>: a pixel's channel quads on an lg-lane group, strips of rows x px pixels, taps in LDS
 *            _WIDE   dwconv7_ln_wide_kernel<nt, rows>: one workgroup of nt threads per strip of rows x px pixels, taps from global memory
 *            _TWO_LAUNCH  dwconv7_kernel<taps_lds, px> (two rows), then the row LayerNorm in place; fp32 storage only (16-bit storage would round the
 *                    un-normalised map between the launches: it takes _TINY on these shapes)
 *            _TINY   dwconv7_ln_kernel: S strips of one row x px pixels per workgroup of nt threads, fp32 output tile in LDS
 *            _CONV   dwconv7_kernel<taps_lds, px, rows> of _FWD
 *            _WGRAD_LDS / _WGRAD_REG  dwconv7_wgrad_lds_kernel (cq channel quads per workgroup) / the register-window dwconv7_wgrad_kernel: S chunks of
 *                    rows_per_chunk rows of the B * H; ws_floats = what this call needs (<= kpf_dwconv7_wgrad_ws_floats); raise_lds: the kernel needs the
 *                    raised dynamic-LDS limit (> 64 KiB) — where the device refuses it, the call takes _WGRAD_REG with that kernel's own chunks
 *   nt = threads of a workgroup, blocks = workgroups of the (first) launch, lds_bytes = its dynamic LDS; fields a family has no use for are 0. */
#define KPF_DW7_OP_LN 0
#define KPF_DW7_OP_FWD 1
#define KPF_DW7_OP_WGRAD 2
#define KPF_DW7_FAMILY_TILE 0
#define KPF_DW7_FAMILY_WAVE 1
#define KPF_DW7_FAMILY_WIDE 2
#define KPF_DW7_FAMILY_TWO_LAUNCH 3
#define KPF_DW7_FAMILY_TINY 4
#define KPF_DW7_FAMILY_CONV 5
#define KPF_DW7_FAMILY_WGRAD_LDS 6
#define KPF_DW7_FAMILY_WGRAD_REG 7
typedef struct kpf_dw7_plan {
  int family, px, rows, taps_lds, lg, nt, nchk, cq, S, rows_per_chunk, raise_lds, reserved;
  long blocks, lds_bytes, ws_floats;
} kpf_dw7_plan;
int kpf_dwconv7_plan(int op, int dtype, int split, int B, int H, int W, int C, kpf_dw7_plan* out);

/*
 * BatchNorm with batch statistics (+ optional ReLU) on NHWC rows x [M][C], forward and backward: nn.BatchNorm2d / BatchNorm1d in
 * train mode as the reference's Residual blocks use them (model/hourglass.py:84-119, `BN -> ReLU -> conv`), C % 4 == 0.
 * forward : mean[c], invstd[c] = 1/sqrt(biased var + eps) are written for the backward; running_mean / running_var (may be NULL)
 *           are updated with `momentum` (unbiased variance), y = [relu]((x - mean) * invstd * w + b).
 * backward: dz = dy (masked by y > 0 when relu; y = the forward output), dx = w*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)),
 *           dw = sum dz*xhat, db = sum dz (dw, db may be NULL).
 * ws >= kpf_bn_ws_floats(M, C) floats; sums are added in a fixed order (run-to-run deterministic).
 */
long kpf_bn_ws_floats(long M, int C);
/* Storage-type generic forms (mixed-precision training): x / dx in x_dtype, y / dy in y_dtype, each KPF_DT_F32 or one 16-bit type
 * (the same on both sides when both are 16-bit); statistics, parameters and all arithmetic stay fp32. */
int kpf_bn_train_forward(const void* x, int x_dtype, const float* w, const float* b, void* y, int y_dtype, float* mean, float* invstd,
                         float* running_mean, float* running_var, float momentum, float eps, int relu, float* ws, long ws_floats, long M, int C,
                         void* stream);
/* addend (x's type and shape; nullable): dx += addend, a second gradient of x — the skip path of a Residual block — folded in */
int kpf_bn_train_backward(const void* dy, const void* x, const void* y, int x_dtype, int y_dtype, const float* mean, const float* invstd,
                          const float* w, const void* addend, void* dx, float* dw, float* db, int relu, float* ws, long ws_floats, long M, int C,
                          void* stream);
/* Training (ABI 17): the embedding sums of a fusion block with their BatchNorms (batch statistics) inside: x [rows][n C], n = n1 + n2 <= 4 sibling Linear outputs side by
 * side (C % 4 == 0, C <= 256), out [rows][C] = relu(S1) (n2 == 0) or relu(relu(S1) + S2) with S1 / S2 the sums of the first n1 / next n2 normalised blocks
 * (model/model.py:254-259, 417-422) — one pass over the pre-activations forward, two backward; w, b, dw, db, running statistics: [n C]; stats [2][n C] = mean, invstd. */
long kpf_bn_ssr_ws_floats(long rows, int C, int n);
int kpf_bn_ssr_forward(const float* x, const float* w, const float* b, float* out, float* stats, float* rmean, float* rvar, float momentum, float eps, float* ws,
                       long ws_floats, long rows, int C, int n1, int n2, void* stream);
int kpf_bn_ssr_backward(const float* dout, const float* out, const float* x, const float* stats, const float* w, const float* b, float* dx, float* dw, float* db, float* ws,
                        long ws_floats, long rows, int C, int n1, int n2, void* stream);
/* Training (ABI 17): y[g][c] = max over the `group` consecutive rows of relu(BN(x)) (batch statistics; fp32 rows x [M][C], M % group == 0) — DESA's `bn -> ReLU ->
 * max over a ball's 64 members` (model/model.py:188-192) — in one pass over the pre-activation (the winner's member index in arg [M / group][C]: first maximum);
 * backward from dmax (rows dmax_ld floats apart): dx dense, dw / db; the BatchNorm sums run over the winners only.  stats [2][C] = mean, invstd. */
long kpf_bn_relu_gmax_ws_floats(long M, int C);
int kpf_bn_relu_gmax_forward(const float* x, const float* w, const float* b, float* y, unsigned char* arg, float* stats, float* rmean, float* rvar, float momentum,
                             float eps, float* ws, long ws_floats, long M, int group, int C, void* stream);
int kpf_bn_relu_gmax_backward(const float* dmax, int dmax_ld, const float* y, const unsigned char* arg, const float* x, const float* stats, const float* w, float* dx,
                              float* dw, float* db, float* ws, long ws_floats, long M, int group, int C, void* stream);
/* Training (ABI 17): out = relu(BN_a(xa) + BN_b(xb)) with batch statistics on fp32 rows [M][C] — DESA's local + feature branches (model/model.py:176-190) — in one
 * pass over the two pre-activations (statistics: two partial + finalize pairs, then ONE element-wise launch), and its backward (masked gradient, both branches'
 * sums, both input gradients: four launches).  stats [4][C] receives mean_a, invstd_a, mean_b, invstd_b (kept for the backward); running statistics nullable and
 * updated like kpf_bn_train_forward's; ws >= kpf_bn2_ws_floats(M, C) floats. */
long kpf_bn2_ws_floats(long M, int C);
int kpf_bn2_add_relu_forward(const float* xa, const float* xb, const float* wa, const float* ba, const float* wb, const float* bb, float* out, float* stats,
                             float* rmean_a, float* rvar_a, float* rmean_b, float* rvar_b, float momentum, float eps, float* ws, long ws_floats, long M, int C,
                             void* stream);
int kpf_bn2_add_relu_backward(const float* dy, const float* out, const float* xa, const float* xb, const float* stats, const float* wa, const float* wb, float* dxa,
                              float* dxb, float* dwa, float* dba, float* dwb, float* dbb, float* ws, long ws_floats, long M, int C, void* stream);

/*
 * Training: data-movement ops of the train-mode forward with a run-to-run deterministic backward (gather form, fixed
 * summation order, no floating-point atomics) — what torch autograd computes with atomics for F.interpolate(bilinear)
 * (model/resnetUnet.py:259), nn.MaxPool2d(3, 2, 1) (model/resnet.py:168), torch.gather on feature rows (model/model.py:297-306) and
 * pointnet2's group_points (model/model.py:174).  NHWC, C % 4 == 0; `dtype` = KPF_DT_F32 / _BF16 / _F16 storage of the activations.
 *   kpf_upsample2x_bwd    dy [B][2H][2W][C] -> dx [B][H][W][C]: the exact transpose of kpf_upsample2x_f32 / _h16.
 *   kpf_maxpool3x3s2_fwd  y [B][OH][OW][C] and tap [B][OH][OW][C] (uint8: winning tap ky*3+kx, first maximum in scan order).
 *   kpf_maxpool3x3s2_bwd  dx[b][iy][ix][c] = sum of dy over the <= 4 windows whose winning tap is (iy, ix).
 *   kpf_row_gather_fwd_f32  out[b][r][:] = sum_{g<G} w[b][r*G+g] * src[b][idx[b][r*G+g]][:]   (src [B][P][C], idx int32 [B][R*G],
 *                           w [B][R*G] or NULL for unit weights, out [B][R][C]).
 *   kpf_row_gather_bwd_f32  dsrc[b][p][:] = sum over entries e ascending with idx[b][e] == p of w[b][e] * dout[b][e/G][:];
 *                           R*G <= 8192 entries and P <= 4096 source rows per image; ws >= kpf_row_gather_ws_ints(B, P, R, G) ints
 *                           (the per-image inverse lists: a stable counting sort of the entries by source row).
 */
int kpf_upsample2x_bwd(const void* dy, void* dx, int dtype, int B, int H, int W, int C, void* stream);
int kpf_maxpool3x3s2_fwd(const void* x, void* y, unsigned char* tap, int dtype, int B, int H, int W, int C, void* stream);
int kpf_maxpool3x3s2_bwd(const void* dy, const unsigned char* tap, void* dx, int dtype, int B, int H, int W, int C, void* stream);
int kpf_row_gather_fwd_f32(const float* src, const int* idx, const float* w, float* out, int B, int P, int R, int G, int C, void* stream);
/* ABI 17: the forward alone for a slice of any width C and layout — element (b, p, c) of the source at b * sb + p * sp + c * sc floats (out [B][R][C] dense; same sum
 * order over g): the 21 weight-logit channels the pose tokens sample (model/model.py:372-376, detached there), read in place from the NCHW offset map. */
int kpf_row_gather_cols_f32(const float* src, long sb, long sp, long sc, const int* idx, const float* w, float* out, int B, int P, int R, int G, int C, void* stream);
long kpf_row_gather_ws_ints(int B, int P, int R, int G);
int kpf_row_gather_bwd_f32(const float* dout, const int* idx, const float* w, float* dsrc, int* ws, long ws_ints, int B, int P, int R, int G, int C,
                           void* stream);
/* Its two halves as separate calls (ABI 13): invert an index tensor once, accumulate for every gather that used it (start = ws, list = ws + B*(P+1);
 * a sub-range of the images is addressed by offsetting both). */
int kpf_row_gather_invert(const int* idx, int* ws, long ws_ints, int B, int P, int R, int G, void* stream);
int kpf_row_gather_accum_f32(const float* dout, const int* start, const int* list, const float* w, float* dsrc, int B, int P, int R, int G, int C, void* stream);

/* Training: LayerNorm over the last axis (nn.LayerNorm / F.layer_norm of convNeXT/convnext.py:43,199-214 and the fusion head's post-LN
 * layers) and GELU(erf) (convNeXT/convnext.py:33), forward and backward.  x [rows][C] fp32, C % 4 == 0, C <= 1024; y in y_dtype (fp32 or the
 * 16-bit operand type of the following GEMM); mean / rstd [rows] are kept for the backward.  backward: dx fp32, dw / db [C] column sums over
 * all rows added in a fixed order through ws (>= kpf_ln_ws_floats(rows, C) floats).  GELU: element-wise on n % 4 == 0 elements of `dtype`. */
/* Training (ABI 16): backward of kpf_ball_group_stacked_f32 towards the features, all three radii in one launch: d3 [B*Jn*64][ld3] (radius i in columns
 * [128 i, 128 i + 128)), start / list = kpf_row_gather_invert of idx [3][B][Jn*64] as 3 B images of P = N + Jn rows (G = 1); dX [B][N][128] for the point
 * features, dnode [B][Jn][128] for the joint features (their gathered rows minus the group sums of the centre subtraction).  Fixed summation order. */
int kpf_ball_group_bwd_f32(const float* d3, int ld3, const int* start, const int* list, float* dX, float* dnode, int B, int N, int Jn, void* stream);
/* Training (ABI 16): y[r][c] = max over the `group` consecutive rows of x [rows*group][C] (model/model.py:192 `.max(2)` over a ball's 64 members), the
 * first maximum's member index kept in arg [rows][C]; backward: dx[r][m][c] = (m == arg[r][c]) ? dy[r][c] : 0, every element written once. */
/* Training (ABI 16): the embedding sums of a fusion block over one channel-stacked tensor y [rows][(n1 + n2) * C]: out [rows][C] = relu(S1) (n2 == 0) or
 * relu(relu(S1) + S2), S1 / S2 = sums of the first n1 / next n2 column blocks (model/model.py:417-422); backward: dy of the same shape. */
int kpf_slices_sum_relu_forward(const float* y, float* out, long rows, int C, int n1, int n2, void* stream);
int kpf_slices_sum_relu_backward(const float* dout, const float* out, const float* y, float* dy, long rows, int C, int n1, int n2, void* stream);
int kpf_group_max_train_forward(const float* x, float* y, unsigned char* arg, long rows, int group, int C, void* stream);
int kpf_group_max_train_backward(const float* dy, int dy_ld /* floats between rows of dy: it may be a column slice of a wider matrix */, const unsigned char* arg, float* dx,
                                 long rows, int group, int C, void* stream);
int kpf_gelu_forward(const void* x, void* y, int dtype, long n, void* stream);
int kpf_gelu_backward(const void* dy, const void* x, void* dx, int dtype, long n, void* stream);

/* Training: the attention core of the 21-token stacks (BertSelfAttention of model/model.py:30-126; multi_head_attention_forward,
 * model/transfusion_head.py:527-546): per (sample, head) P = softmax(scale * Q K^T), ctx = dropout(P) V.  q, k, v, ctx, dq, dk, dv are rows
 * [B*T][ld] fp32 with head h in channels [h*hd, (h+1)*hd) (the projections' own layout: no head transposes); T = 21, hd = 32.  P
 * [B][H][T][T] fp32 and the keep mask M (bytes) are kept for the backward.  p_drop > 0: masks from a hash of (rng[0] = seed, rng[1] =
 * counter advanced by the host once per forward, call_id, element); rng is a device pointer to two int64. */
/* q / k / v (dq / dk / dv) have row stride ld, ctx (dctx) its own row stride ldc (ABI 13): the three projections may be column slices of one [rows][3C]
 * GEMM output (ld = 3C, ldc = C); separate dense tensors pass ldc = ld. */
int kpf_attn21_forward(const float* q, const float* k, const float* v, float* ctx, float* P, unsigned char* M, int B, int T, int H, int hd, int ld, int ldc,
                       float scale, float p_drop, const long* rng, int call_id, void* stream);
int kpf_attn21_backward(const float* dctx, const float* q, const float* k, const float* v, const float* P, const unsigned char* M, float* dq, float* dk,
                        float* dv, int B, int T, int H, int hd, int ld, int ldc, float scale, float p_drop, void* stream);

/* Training: dX[b] (P x C) = A[b]^T (P x J) @ dOut[b] (J x C) for small J (<= 64; J = 21 joints): the operand gradient of the per-sample
 * products of model/model.py:318-320 and 336-341 (a K = J batched GEMM the library handles badly).  fp32, C % 4 == 0, J * C * 4 B <= 64 KB. */
int kpf_bmm_small_k_dx(const float* A, const float* dOut, float* dX, int B, int J, int P, int C, void* stream);
/* round 5 (ABI 14): the other two products of the pair — out[b] = A[b] (J x P) @ X[b] (P x C) (J <= 24, C % 4 == 0) and dA[b] = dOut[b] (J x C) @ X[b]^T — what
   torch.bmm computed in `joint_feat = img2joint @ img_feat` (model/model.py:318-320) and the gated reduction (model/model.py:336-341) of the training step and in
   their autograd backward; fixed summation order. */
int kpf_bmm_small_k_fwd(const float* A, const float* X, float* out, int B, int J, int P, int C, void* stream);
int kpf_bmm_small_k_da(const float* dOut, const float* X, float* dA, int B, int J, int P, int C, void* stream);

/* Training: the dense-stage loss (train.py:211-224 with GFM.joint2offset / offset2joint_weight, util/generateFeature.py:59-84,166-195, and
 * model/loss.py's SmoothL1): pd [B][5J][F][F] fp32 NCHW (3J unit offsets (j, xyz), J heat maps, J weight logits), img [B][1][S][S], uvd_gt
 * [B][J][3].  forward writes part [B][J][2] = per-(sample, joint) sums of the element losses (pixel term over its 4 channels, coordinate
 * term over its 3 coordinates): loss_pixel = sum(part[..., 0]) / (B*4J*F*F), loss_coord = sum(part[..., 1]) / (B*J*3).  backward: grad2 =
 * device pointer to {dL/dloss_pixel, dL/dloss_coord}; every element of dpd [B][5J][F][F] is written.  F*F <= 1024, S % F == 0. */
int kpf_dense_loss_forward(const float* pd, const float* img, const float* uvd_gt, float* part, int B, int J, int F, int S, float kernel_size, void* stream);
int kpf_dense_loss_backward(const float* pd, const float* img, const float* uvd_gt, const float* grad2, float* dpd, int B, int J, int F, int S,
                            float kernel_size, void* stream);

/* Training: the rest of the loss of train.py:225-261 (two launches forward, one backward): SmoothL1 (model/loss.py) between the four
 * fusion-block joint sets joints4[i] [B][J][3] and xyz_gt, the two spatial-weight terms against GFM.joint2heatmap(uvd_gt[..., :2])
 * (util/generateFeature.py:584-600) divided by its global maximum, the epoch gate of train.py:251 read from a device scalar, the weights and
 * the total, together with the dense stages' partial sums dense0 / dense1 (kpf_dense_loss_forward's part; nullable).
 * joints4 / sw2 / djoints4 / dsw2: HOST arrays of device pointers (entries nullable = term absent / gradient not wanted); sw2[t] element
 * (b, j, p = y*F + x) at b*sw_strides6[3t] + j*sw_strides6[3t+1] + p*sw_strides6[3t+2]; epoch: device float (nullable: gates = 1);
 * cfg9 (host) = {std, sigma0, sigma1, coord_weight, deconv_weight, spatial_weight0, spatial_weight1, spatial_epoch0, spatial_epoch1};
 * sp_part: 2*B*J floats of workspace; out16: [0] loss, [1..4] pixel_0 coord_0 pixel_1 coord_1, [5..8] coord_2..5, [9..10] spatial_0..1
 * (weighted, gated), [12..13] gates, [14..15] the heat maps' maxima (read again by the backward).
 * backward: g = device pointer to dL/dloss; writes djoints4[i], dsw2[t] (same strides as sw2[t]) and gdense2 = {g*deconv_weight,
 * g*coord_weight}, the grad2 of kpf_dense_loss_backward. */
int kpf_loss_tail_forward(const float* dense0, const float* dense1, const float* const* joints4, const float* xyz_gt, const float* uvd_gt,
                          const float* const* sw2, const long* sw_strides6, const float* epoch, const float* cfg9, float* sp_part, float* out16,
                          int B, int J, int F, void* stream);
int kpf_loss_tail_backward(const float* const* joints4, const float* xyz_gt, const float* uvd_gt, const float* const* sw2, const long* sw_strides6,
                           const float* cfg9, const float* out16, const float* g, float* const* djoints4, float* const* dsw2, float* gdense2,
                           int B, int J, int F, void* stream);

/* Training: one-launch packing of a reference-layout weight w [N][Cin][KH][KW] (src_dtype: KPF_DT_F32 master, or a 16-bit copy) into an
 * operand of kpf_conv2d_f32 / _h16 (dst_dtype; fp32 -> 16-bit rounds to nearest even), rows zero-padded to Kp:
 *   mode 0  forward rows        dst [n_pad][Kp], k = (ky, kx, c)
 *   mode 1  data-gradient rows  dst [Cin][Kp],   k = (ky, kx, n < n_pad) with mirrored taps (transposed convolution, stride-1 form)
 *   mode 2  patchify data-grad  dst [(ky, kx, c)][Kp], k = n < n_pad        (kernel == stride convolutions: a GEMM + pixel un-shuffle;
 *                               with Cin = 1: the depthwise tap table [KH*KW][C] of kpf_dwconv7_f32)
 *   mode 3  mode 2 with the taps mirrored (the depthwise convolution's data gradient) */
int kpf_pack_conv_weight(const void* w, int src_dtype, void* dst, int dst_dtype, int N, int Cin, int KH, int KW, int mode, int n_pad, int Kp,
                         void* stream);

/* All operands of an iteration in ONE launch: `descs_device` is an array of `ndesc` descriptors in DEVICE memory, sorted by
 * first_block; descriptor i owns workgroups [first_block, first_block + kpf_pack_desc_blocks(i)) of the `total_blocks` launched.
 * Fields as the arguments of kpf_pack_conv_weight (rows = destination rows: n_pad / Cin / KH*KW*Cin for mode 0 / 1 / 2-3). */
typedef struct kpf_pack_desc {
  const void* src;
  void* dst;
  int N, Cin, KH, KW, mode, n_pad, Kp, rows;
  int src_dtype, dst_dtype, first_block, reserved; /* reserved (ABI 13): 0, or the destination's row stride in elements when it exceeds Kp (the operand
                                                      is a column range of a wider stacked matrix); mode 4 (ABI 13): a vector of N elements, rows = 1 */
} kpf_pack_desc;
int kpf_pack_conv_weights_multi(const kpf_pack_desc* descs_device, int ndesc, int total_blocks, void* stream);
/* workgroups descriptor d occupies in that launch (first_block of the next descriptor = first_block + this; ABI 13: the kernel serves 1x1 transposes,
 * k x k rows, tap tables and k x k data-gradient rows with LDS-staged forms of their own geometry) */
long kpf_pack_desc_blocks(const kpf_pack_desc* d);

/* Training: AdamW (train.py:84-91) over many tensors in ceil(n / KPF_ADAMW_BATCH) launches.  descs: HOST array (p, m, v updated in place;
 * g read; all fp32, n elements each; first_block is set by the call); the learning rate is *lr_dev when lr_dev is non-null (device
 * scalar: a captured iteration follows the scheduler) else lr_host; *step_dev is the number of steps taken BEFORE this one (device float;
 * the caller increments it afterwards).  Arithmetic of torch.optim.AdamW(fused=True): decoupled weight decay, bias corrections from
 * step + 1, no amsgrad. */
#define KPF_ADAMW_BATCH 320 /* (round 6: 80 -> 320, a 15-KB kernel-argument segment: the ~1100 tensors of a paired ConvNeXt-T KPFusion take 4 launches instead of 14) */
typedef struct kpf_adamw_desc {
  float* p;
  const float* g;
  float* m;
  float* v;
  long n;
  int first_block, reserved;
} kpf_adamw_desc;
int kpf_adamw_step_multi(const kpf_adamw_desc* descs, int n, const float* lr_dev, float lr_host, const float* step_dev, double beta1, double beta2, float eps,
                         float weight_decay, void* stream);
/* round 5 (ABI 14): loss scaling for fp16 mixed-precision training, on the device (what torch.cuda.amp.GradScaler does around train.py:262-264; a captured
 * iteration keeps following it).  kpf_grad_finite_check_multi: *found_dev |= 1 when any gradient of the descriptors (p / m / v unused) holds an inf or a nan.
 * kpf_adamw_step_multi_scaled: kpf_adamw_step_multi on g * *inv_scale_dev, or a no-op when *skip_dev != 0 (either pointer may be null).
 * kpf_loss_scale_update: found -> scale *= backoff and the growth tracker restarts; otherwise *step_dev += 1 (nullable) and scale *= growth every `interval` clean
 * steps; scale stays in [1, 2^24], *inv_scale_dev = 1 / scale, *found_dev = 0 for the next iteration. */
int kpf_grad_finite_check_multi(const kpf_adamw_desc* descs, int n, int* found_dev, void* stream);
int kpf_adamw_step_multi_scaled(const kpf_adamw_desc* descs, int n, const float* lr_dev, float lr_host, const float* step_dev, double beta1, double beta2,
                                float eps, float weight_decay, const float* inv_scale_dev, const int* skip_dev, void* stream);
int kpf_loss_scale_update(float* scale_dev, float* inv_scale_dev, int* tracker_dev, int* found_dev, float* step_dev, float growth, float backoff, int interval,
                          void* stream);

/* Training: the weight (and bias) gradients of MANY Linear layers over few rows in one launch per KPF_WGRAD_GROUP_BATCH problems:
 * dw[N][K] = dy[M][N]^T x[M][K], db[N] = column sums of dy (db nullable), fp32, N % 4 == K % 4 == 0, rows contiguous.  A workgroup owns a
 * 64 x 64 tile of one problem and walks all M rows (no split, no reduce launch) — meant for M up to ~1000 (the 21-token stacks of the
 * fusion head: M = 21 B), where a launch pair per layer costs more than the arithmetic; the row range is still summed in the splits of
 * kpf_conv2d_wgrad and the split sums in split order, so both forms return the same bits.  descs: HOST array. */
#define KPF_WGRAD_GROUP_BATCH 64
typedef struct kpf_wgrad_group_desc {
  const float* dy;
  const float* x;
  float* dw;
  float* db;
  int M, N, K, first_block; /* (first_block, sps: set by the call) */
  int sps, ldy;             /* ldy: floats between rows of dy (0 = N; ABI 13: dy may be a column slice of a wider matrix, e.g. one of q | k | v) */
} kpf_wgrad_group_desc;
int kpf_linear_wgrad_grouped(const kpf_wgrad_group_desc* descs, int n, void* stream);

/* Training: the column-sum reduce behind every LayerNorm / layer-scale backward (d gamma, d beta) for many layers in one launch.
 * kpf_ln_train_backward / kpf_layer_scale_backward / kpf_drop_add_ln_backward with desc != NULL run everything but that reduce, leave the
 * per-workgroup partial sums in `ws` (which must stay alive) and fill `desc`: dw / db (dgamma) are UNWRITTEN until
 * kpf_colsum_reduce_grouped(descs: HOST array) performs the reduces, KPF_COLSUM_BATCH per launch, with the arithmetic of the immediate form
 * (same bits).  desc == NULL: the call launches its own reduce. */
#define KPF_COLSUM_BATCH 96
typedef struct kpf_colsum_desc {
  const float* part; /* [nblk][2][C] */
  float* dw;         /* column sums of plane 0 */
  float* db;         /* column sums of plane 1 */
  int nblk, C, first_block;
  int reserved;      /* ABI 17: that many floats behind db[C - 1] are set to zero (0: none) — the sum over the batch of a [B][T*C] gradient of the first T rows of an
                        embedding table [L][C] written as the table's whole gradient: part = the [B][T*C] tensor read as [B][2][T*C/2], dw = the table's gradient,
                        db = dw + T*C/2, reserved = (L - T) * C (model/model.py:84 position embeddings; model/transfusion_head.py:150-152) */
} kpf_colsum_desc;
int kpf_colsum_reduce_grouped(const kpf_colsum_desc* descs, int n, void* stream);

/* LayerNorm over fp32 rows of C (C % 4 == 0, C <= 1024), y in y_dtype, mean / rstd [rows] kept for the backward (dy in dy_dtype; dx fp32; dw / db summed
 * in a fixed order through ws).  G parameter sets (ABI 13): row r is normalised with set r % G, i.e. w, b, dw, db hold [G][C] — what a LayerNorm over
 * each of the G channel groups of a [pixels][G*C] tensor is when that tensor is read as [pixels*G][C] rows (the paired backbones of the training
 * step).  G in {1, 2, 4}, rows % G == 0; G = 1 is the plain LayerNorm.  ws_floats >= kpf_ln_ws_floats(rows, G*C).  desc: nullable, see above (C -> G*C). */
long kpf_ln_ws_floats(long rows, int C);
int kpf_ln_train_forward(const float* x, const float* w, const float* b, void* y, int y_dtype, float* mean, float* rstd, long rows, int C, int G,
                         float eps, void* stream);
int kpf_ln_train_backward(const void* dy, int dy_dtype, const float* x, const float* mean, const float* rstd, const float* w, float* dx, float* dw,
                          float* db, float* ws, long ws_floats, long rows, int C, int G, kpf_colsum_desc* desc, void* stream);

/* y = LayerNorm(h + dropout(o)) in one launch each way (ABI 13; model/model.py:30-126: dense -> dropout -> residual add -> LayerNorm, both halves of a
 * BERT layer).  fp32 rows of C (C % 4 == 0, C <= 1024); xs = h + dropout(o) [rows][C], the keep mask [rows][C] bytes (NULL when p_drop == 0) and
 * mean / rstd [rows] are kept for the backward; rng: the device-resident (seed, counter) pair of kpf_attn21_forward, call_id a per-site constant.
 * backward: dh = d xs, d_o = d xs * mask / (1 - p), dw / db [C]; ws_floats >= kpf_ln_ws_floats(rows, C); desc as kpf_ln_train_backward. */
int kpf_drop_add_ln_forward(const float* o, const float* h, const float* w, const float* b, float* xs, float* y, unsigned char* mask, float* mean, float* rstd,
                            long rows, int C, float eps, float p_drop, const long* rng, int call_id, void* stream);
int kpf_drop_add_ln_backward(const float* dy, const float* xs, const float* mean, const float* rstd, const float* w, const unsigned char* mask, float* dh,
                             float* d_o, float* dw, float* db, float* ws, long ws_floats, long rows, int C, float p_drop, kpf_colsum_desc* desc, void* stream);
/* Layer scale + residual of the ConvNeXt block, out = x + gamma * y (convNeXT/convnext.py:48-51): x / out / g fp32 [rows][C], y / dy in
 * y_dtype (fp32 or the 16-bit GEMM storage type), gamma / dgamma [C]; C % 4 == 0, C <= 1024.  backward: dy = g * gamma, dgamma = column sums of
 * g * y added in a fixed order through ws.  G parameter sets (G in {1, 2, 4}, rows % G == 0; same row-view convention as kpf_ln_train_backward:
 * rows counts [rows][C] rows of a [rows / G][G*C] tensor, gamma / dgamma hold [G][C]); ws_floats >= kpf_layer_scale_ws_floats(rows, G*C).
 * The forward needs no G (call it with C := G*C).  desc: nullable, see above. */
long kpf_layer_scale_ws_floats(long rows, int C);
int kpf_layer_scale_forward(const float* x, const void* y, int y_dtype, const float* gamma, float* out, long rows, int C, void* stream);
int kpf_layer_scale_backward(const float* g, const void* y, int y_dtype, const float* gamma, void* dy, float* dgamma, float* ws, long ws_floats,
                             long rows, int C, int G, kpf_colsum_desc* desc, void* stream);

/* Training (ABI 16): the four BERT layers of a KP_Interaction_TR stack (21 tokens x 128, 4 heads x 32, intermediate 16, GELU-erf, post-LN eps 1e-12,
 * hidden / attention dropout p_drop) as ONE launch per direction — replaces model/model.py:30-126 (transformers' BertEncoder under .train()) between the
 * embedding Linear and the cls_head / residual heads.  csrc/kpf_trstack.hip: one workgroup per sample, weights streamed by dedicated loader waves from the
 * parameter tensors as they lie in memory ([N][K] fp32, 16-byte aligned).
 *   forward : H[0] = dropout(e + pos), then the four layers; e [B][21][128], pos [21][128]; param_table = DEVICE array of 4 x 16 pointers per layer in the order
 *             Wq bq Wk bk Wv bv Wo bo ln1.w ln1.b Wi bi Wo2 bo2 ln2.w ln2.b; everything the backward needs goes to `save`
 *             (kpf_tr_stack_save_floats(B) floats); the stack's output [B][21][128] is save + kpf_tr_stack_out_offset(B).
 *             rng: the device-resident (seed, counter) pair of kpf_attn21_forward; call0: first of 13 consecutive dropout call ids.
 *   backward: dh [B][21][128] -> dE [B][21][128] (gradient of e, and of pos after a sum over B); every Linear's dY goes to `dys`
 *             (kpf_tr_stack_dy_floats(B)) beside the X kept in `save` (kpf_tr_stack_offset(B, layer, which): which 0-3 = X of q|k|v / attention output /
 *             intermediate / output in `save`, 4-7 = dqkv [M][384] / d(attention output) / d(intermediate) [M][16] / d(output) in `dys`) for
 *             kpf_linear_wgrad_grouped; LayerNorm parameter gradients leave as per-sample partial sums parts[layer][ln][B][2][128]
 *             (kpf_tr_stack_part_floats(B); a kpf_colsum_desc with nblk = B, C = 128 each).  Dropout masks are recomputed from the (seed, counter) the
 *             forward stored in `save`.  Fixed summation order: bit-identical replays. */
/* Training (ABI 16): the decoder layer of the fusion block (updatedDecoder layer 3, model/transfusion_head.py:137-173, 437-554: cross attention of 21 query tokens over 21
 * key tokens, post-LN eps 1e-5, ReLU feed-forward of width 128, dropout) as one launch each way on the engine of kpf_tr_stack_train_*.  query / key [B][21][128];
 * param_table: DEVICE array of 14 pointers — in_proj_weight [384][128], in_proj_bias, out_proj.weight, out_proj.bias, norm2.weight, norm2.bias, linear1.weight, linear1.bias,
 * linear2.weight, linear2.bias, norm3.weight, norm3.bias, self_posembed [21][128], cross_posembed [21][128]; the output is save + kpf_xattn_train_offset(B, 5).
 * backward: dquery (both paths), dqe / dke = gradients of query + qpos / key + kpos (dkey = dke; the position tables' gradients are their sums over B); dys
 * (kpf_xattn_train_dy_floats) receives dqkv [M][384] | d out_proj [M][128] | d linear1 | d linear2 for the weight gradients (X operands: kpf_xattn_train_offset
 * 0 qe, 1 ke, 2 ctx, 3 x, 4 hidden); parts [2][B][2][128] the LayerNorm partial sums (norm2, norm3).  call0: first of 4 consecutive dropout call ids; mma as above. */
long kpf_xattn_train_save_floats(int B);
long kpf_xattn_train_dy_floats(int B);
long kpf_xattn_train_offset(int B, int which);
int kpf_xattn_train_forward(const float* query, const float* key, const void* param_table, float* save, long save_floats, int B, float p_drop, const long* rng,
                            int call0, int mma, void* stream);
int kpf_xattn_train_backward(const float* dout, const void* param_table, const float* save, float* dquery, float* dqe, float* dke, float* dys, float* parts, int B,
                             float p_drop, int call0, int mma, void* stream);
int kpf_tr_stack_set_stamps(void* stamps64 /* tuning aid: 64 device uint64 slots for in-kernel wall-clock stamps of workgroup 0; NULL = off */);
long kpf_tr_stack_save_floats(int B);
long kpf_tr_stack_out_offset(int B);
long kpf_tr_stack_dy_floats(int B);
long kpf_tr_stack_part_floats(int B);
long kpf_tr_stack_offset(int B, int layer, int which);
/* mma: 0 = fp32 products on v_mfma_f32_16x16x4_f32 (the fp32 step), 1 / 2 = operands rounded to bf16 / f16 in registers, fp32 accumulation (the mixed-precision step:
 * what torch.autocast does to these Linears); softmax, LayerNorm, GELU, residual sums and everything stored stay fp32. */
int kpf_tr_stack_train_forward(const float* e, const float* pos, const void* param_table, float* save, long save_floats, int B, float p_drop, const long* rng,
                               int call0, int mma, void* stream);
int kpf_tr_stack_train_backward(const float* dh, const void* param_table, const float* save, float* dE, float* dys, float* parts, int B, float p_drop,
                                int call0, int mma, void* stream);

/* Training: the two analytic maps of a fusion block (model/model.py:300-336) with their gradients towards the joints, one launch each:
 * hm[b][j][y][x] = GFM.joint2heatmap(uvd[..., :2], std, F, sigma) (util/generateFeature.py:584-600), duvd [B][J][3] (z component 0);
 * gam[b][j][p] = 1 / (10 |pix_xyz[b][p] - joint_xyz[b][j]|^2 + 1) (dataloader/loader.py:791-819), djoint [B][J][3].  fp32, contiguous. */
int kpf_joint_heatmap_forward(const float* uvd, float* hm, int B, int J, int F, float std_, float sigma, void* stream);
int kpf_joint_heatmap_backward(const float* uvd, const float* dhm, float* duvd, int B, int J, int F, float std_, float sigma, void* stream);
int kpf_geom_gate_forward(const float* pix_xyz, const float* joint_xyz, float* gam, int B, int J, int P, void* stream);
int kpf_geom_gate_backward(const float* pix_xyz, const float* joint_xyz, const float* dgam, float* djoint, int B, int J, int P, void* stream);

/* The same map with the joints given in crop coordinates uvd in [-1, 1]^3 (ABI 13): the uvd -> camera -> cube-normalised xyz transform of
 * dataloader/loader.py:775-789 (half_size = img_size / 2, flip = +-1) runs inside the kernel (in double: one joint per workgroup) and the backward returns d/d(uvd).
 * par16 [B][16] = [M^-1 rows 0 and 1 (6) | fx fy u0 v0 (4) | centre xyz (3) | cube xyz (3)] per sample.  Replaces model/model.py:318-326. */
int kpf_geom_gate_uvd_forward(const float* pix_xyz, const float* joint_uvd, const float* par16, float* gam, int B, int J, int P, float half_size, float flip,
                              void* stream);
int kpf_geom_gate_uvd_backward(const float* pix_xyz, const float* joint_uvd, const float* par16, const float* dgam, float* djoint_uvd, int B, int J, int P,
                               float half_size, float flip, void* stream);

/* Device-side RGB-D preprocessing (ABI 18): keypointfusion_amd/preprocess.py::prepare_rgbd for a batch of frames, and the un-crop of predicted joints
 * (reference: demo_RGBD.py:72-108, :121-147).  Every argument is a device buffer, so a captured graph picks up new frames, boxes and seeds at replay; grids
 * depend on B, S and n only; a sample's result does not depend on B.  Integer decisions and both images are bit-equal to the host path.
 *
 * kpf_prep_crop_u16: rgb [B][Hs][Ws][3] uint8 (channel order kept), depth [B][Hs][Ws] uint16 mm, bbox [B][4] double (x, y, w, h; top-left), cam [B][4] double
 * (fx fy u0 v0), cube [B][3] double (mm).  The stored image is the window [y0, y0 + Hs) x [x0, x0 + Ws) of a logical H x W frame whose other pixels read as
 * zero (a whole frame: x0 = y0 = 0, H = Hs, W = Ws).  One workgroup per sample: centre of mass of the valid depth in the box (64-bit integer sums, exact) ->
 * pixel bounds of the cube -> nearest-neighbour crop with zero padding, letterboxed into S x S -> z-clamp (near plane truncated to uint16) -> normalised depth.
 * -> img [B][1][S][S], img_rgb [B][3][S][S] (/ 255), center [B][3], M [B][3][3], cube_out [B][3], cam_para [B][4] (float: the model's inputs), and the record
 * com [B][3] double (u, v, d mm), bounds [B][6] int (xs, xe, ys, ye, resize width, resize height), M64 [B][3][3] double (M before its rounding to float).
 * S * S <= 16384. */
int kpf_prep_crop_u16(const unsigned char* rgb, const unsigned short* depth, const double* bbox, const double* cam, const double* cube, int B, int Hs, int Ws,
                      int x0, int y0, int H, int W, int S, float* img, float* img_rgb, float* center, float* M, float* cube_out, float* cam_para, double* com,
                      int* bounds, double* M64, void* stream);

/* kpf_prep_pcl_sample: depth_to_pcl + sample_points on kpf_prep_crop_u16's outputs (img, center, M64) and the same cube / cam.  The foreground pixels in
 * row-major order (np.where) are the candidates; N = their number.  n of them are drawn without replacement IN RANDOM ORDER: (key, candidate) pairs, key = a
 * counter hash of (seed[b], candidate), are sorted in LDS and the first n taken.  0 < N < n: every candidate floor(n / N) times, n mod N distinct ones once
 * more, the n slots shuffled.  N == 0: zeros, index -1.  -> pcl [B][n][3] float (clipped to [-1, 1]), pcl_index [B][n] int (candidate index), pcl_count [B]
 * int (N).  cand_pts: NULL, or [B][S * S][3] float receiving every candidate's point at its candidate index (rows >= N untouched): tests and debugging.
 * seed [B] 64-bit.  n <= S * S <= 16384, and (pow2ceil(S * S) + pow2ceil(n)) * 8 + 128 bytes of LDS must fit 160 KiB. */
int kpf_prep_pcl_sample(const float* img, const float* center, const double* M64, const double* cube, const double* cam, const long long* seed, int B, int S,
                        int n, float* pcl, int* pcl_index, int* pcl_count, float* cand_pts, void* stream);

/* kpf_prep_uncrop_f32: joints [B][J][3] normalised to the cube + center, M, cube_out, cam_para of kpf_prep_crop_u16 -> crop_px [B][J][3] (u, v in crop
 * pixels, d mm: preprocess.project_to_crop) and frame_px [B][J][3] (u, v in frame pixels: preprocess.uncrop_points).  Double inside, one thread per joint. */
int kpf_prep_uncrop_f32(const float* joints, const float* center, const float* M, const float* cube, const float* cam, int B, int J, float* crop_px,
                        float* frame_px, void* stream);

int kpf_prep_set_stamps(void* stamps64 /* tuning aid: [B][8] device uint64 slots for in-kernel wall-clock stamps (100 MHz) of every sample's workgroup:
                                            kpf_prep_crop_u16 0 start, 1 geometry, 2 gather, 3 end; kpf_prep_pcl_sample 4 start, 5 compacted, 6 sorted, 7 end;
                                            NULL = off.  Synchronises with the device: not for captured code */);

/* Device-resident evaluation (ABI 20): the per-batch figures of the reference's test loop (train.py:326-399, :470-488; util/generateFeature.py:676-703;
 * util/eval_utils.py:38-81) accumulated in device memory.  Every argument but `stages` is a device buffer, no entry synchronises or allocates, and the
 * arithmetic order below is part of the interface: results do not depend on B, on the grid or on a graph replay.
 *
 * kpf_eval_errors_f32: stages = HOST array of S <= 8 device pointers, each the normalised joints [B][J][3] float of one stage (read at the call: the pointers
 * travel to the kernel by value); gt [B][J][3] float, cube [B][3] float (mm); score_index NULL (Jsel == J) or Jsel int joint indices in [0, J) (NYU: 14 of 23).
 * One wave64 per (sample, stage), one lane per joint, J <= 64; all arithmetic in double from the float inputs, no contraction:
 *   plain:   e_j = sqrt(dx^2 + dy^2 + dz^2), d = (p_j - g_j) * (cube / 2), summed left to right, rounded ONCE to float (the crop centre cancels and is not added);
 *   aligned: the same formula after the Umeyama similarity alignment of p onto g over ALL J joints (selection comes after the alignment, as in the
 *            reference): centroids = sum / J, H = A0^T B0 / J, var = |A0|^2 / J, 3 x 3 SVD of H by 8 sweeps of cyclic Jacobi on H^T H (pairs (0,1), (0,2),
 *            (1,2)), V = its eigenvectors by descending eigenvalue with v3 = v1 x v2, u1 = H v1 / |H v1|, u2 = H v2 orthogonalised against u1 and normalised,
 *            u3 = u1 x u2, third singular value SIGNED s3 = u3^T H v3 (negative = the reflection branch d = -1), R = V U^T, scale = (s1 + s2 + s3) / var,
 *            aligned_j = scale * R a0_j + centroid(g).
 *   Every cross-lane sum is the 64-lane xor butterfly (offsets 32, 16, .. 1) with lanes >= J holding +0.0.
 * -> err [2][S][B][Jsel] float: plain, then aligned.  When every predicted joint of a sample is the same point, var and H are 0 and that sample's ALIGNED
 * errors are NaN (0 / 0, as in the reference); its plain errors and every other sample are unaffected.  A rank-deficient H with var > 0 gives finite results. */
int kpf_eval_errors_f32(const float* const* stages, int S, const float* gt, const float* cube, const int* score_index, int B, int J, int Jsel, float* err,
                        void* stream);

/* kpf_eval_accumulate: err of the call above; valid NULL or [B] bytes (0 drops a sample: the padding of a last partial batch at fixed B); thresholds [T]
 * double (np.linspace on the host, so that they carry numpy's bits).  One workgroup per stage, every output element owned by one thread, no atomics:
 *   n_samples [1] += valid samples; n_batches [1] += 1 unless no sample is valid (then nothing at all is added)          (64-bit integers)
 *   sum_err, sum_pa [S][Jsel] double: the running sum continued sequentially, x = x + (double)err[b][j] for the valid b = 0 .. B-1 in order
 *   sum_batch_mean, sum_batch_pa_mean [S] double += (sequential sum from 0.0 over valid b = 0 .. B-1, j = 0 .. Jsel-1 inner) / (valid * Jsel): the batch
 *       means the reference averages (error_list / PA_error_list, train.py:381-397)
 *   pck, pck_pa [S][Jsel][T] 64-bit integers += number of valid b with (double)err[b][j] <= thresholds[t] (numpy's comparison on the logged float; NaN never counts)
 * 2 * B * Jsel * 4 + B bytes of LDS must fit 64 KiB. */
int kpf_eval_accumulate(const float* err, const unsigned char* valid, const double* thresholds, int S, int B, int Jsel, int T, long long* n_samples,
                        long long* n_batches, double* sum_err, double* sum_pa, double* sum_batch_mean, double* sum_batch_pa_mean, long long* pck,
                        long long* pck_pa, void* stream);

/* Several tracks on one stored frame (ABI 21): kpf_prep_crop_u16 with a frame index.  rgb [F][Hs][Ws][3], depth [F][Hs][Ws]; frame_index [B] int (device):
 * sample b reads stored frame frame_index[b].  The caller keeps the values in [0, F) (preprocess_gpu.make_frame_index refuses others on the host); the kernel
 * clamps them as well, so that no index reads out of bounds.  Everything else, and every result, as kpf_prep_crop_u16 — which is this kernel without an index
 * (sample b reads frame b). */
int kpf_prep_crop_u16_indexed(const unsigned char* rgb, const unsigned short* depth, const int* frame_index, int F, const double* bbox, const double* cam,
                              const double* cube, int B, int Hs, int Ws, int x0, int y0, int H, int W, int S, float* img, float* img_rgb, float* center, float* M,
                              float* cube_out, float* cam_para, double* com, int* bounds, double* M64, void* stream);

/* Tracking step (ABI 21): ONE launch behind the forward that takes the place of kpf_prep_uncrop_f32 in a tracked video stream and leaves the NEXT frame's box in
 * device memory (keypointfusion_amd/tracking.py).  joints [B][J][3] float normalised to the cube; center, M, cube, cam_para: the float outputs of
 * kpf_prep_crop_u16; pcl_count [B] int of kpf_prep_pcl_sample.  One wave64 per sample, one lane per joint, J <= 64; grid = B; no allocation, no
 * synchronisation, no atomics; contraction off.
 *   crop_px, frame_px [B][J][3]: the expressions and the bits of kpf_prep_uncrop_f32.   cam_mm [B][J][3] = ((j * cube) / 2) + center in float, each step rounded
 *   (camera space, mm: demo_RGBD.py:133).   bbox_used [B][4] double: a copy of the box this frame was cropped with.
 *   Box rule = the reference loader's get_bbox + process_bbox (dataloader/loader.py:1250-1251, :1432-1480), restated by tracking.next_bbox: min / max of the
 *   STORED float frame_px u and v by xor butterflies (lanes >= J hold +-inf), then in FLOAT, every operation rounded: c = (lo + hi) / 2, w = (hi - lo) * expansion,
 *   x0 = c - 0.5 w, x1 = c + 0.5 w, bx = x0, bw = x1 - x0 (the same for y); then in DOUBLE: X1 = max(0, bx), Y1 = max(0, by), X2 = min(frame_w - 1, X1 +
 *   max(0, bw - 1)), Y2 likewise; no box unless bw * bh > 0 and X2 >= X1 and Y2 >= Y1; w = X2 - X1, h = Y2 - Y1, centre = X1 + w / 2, Y1 + h / 2, the shorter
 *   side raised to the longer, box = (cx - w / 2, cy - h / 2, w, h).
 *   status [B] int, bits: 1 the rule gave no box; 2 pcl_count[b] == 0 (the crop had no foreground: the prediction means nothing); 4 a frame_px u or v is not
 *   finite (the rule is not evaluated).
 * State, updated in place: bbox [B][4] double — in: this frame's box, out: the next frame's (status 0) or unchanged (status != 0); lost [B] int = 0 (status 0) or
 * + 1; seed [B] 64-bit += seed_stride.  A sample's outputs do not depend on B, on its position in the batch or on a graph replay. */
int kpf_track_step_f32(const float* joints, const float* center, const float* M, const float* cube, const float* cam_para, const int* pcl_count, int B, int J,
                       int frame_w, int frame_h, float expansion, long long seed_stride, double* bbox, long long* seed, int* lost, float* crop_px,
                       float* frame_px, float* cam_mm, double* bbox_used, int* status, void* stream);

/* Preprocessing by the dataset protocol (ABI 23): annotations in, the model's inputs AND the labels out — keypointfusion_amd/preprocess.py::prepare_annotated
 * (reference: dataloader/loader.py:1113-1204 DexYCB and :1296-1416 HO3D, test branch, flip = 1).  The crop is cut around an ANNOTATED 3-D centre instead of a
 * box's centre of mass, left hands are mirrored, and everything up to the integer bounds is FLOAT arithmetic (the annotations and intrinsics are float32 in
 * the reference), every operation an IEEE +, -, *, / rounded once, no contraction.
 *
 * kpf_prep_annot_u16: rgb, depth, frame_index / F (NULL / F >= B: sample b reads frame b), the window and S as kpf_prep_crop_u16[_indexed]; joints_mm
 * [B][J][3] float (camera space, mm, the model's joint order; NULL: no ground truth, the labels are zeros), cam32 [B][4] float (fx fy u0 v0), center_xyz
 * [B][3] float (NULL: the mean of the joints; joints_mm and center_xyz are not both NULL), mirror [B] bytes (non-zero: a left hand), cube [B][3] double.
 * One workgroup of 1024 threads per sample, J <= 64.  Wave 0, one lane per joint: uvd = (x * fx / z + u0, y * fy / z + v0, z); mirrored: u = (W - u) - 1;
 * xyz = ((u - u0) * d / fx, (v - v0) * d / fy, d).  One lane: centre = center_xyz, or the xyz rows summed IN ORDER j = 0 .. J-1 from 0 and divided by J;
 * center_uvd = its projection; bounds xs = (int)floor((u * d / fx - cube_x / 2) / d * fx + 0.5) (xe with +, ys / ye with v, fy, cube_y), z range d -+ cube_z
 * / 2, all in float; from the integer bounds on as kpf_prep_crop_u16 (M in double).  A mirrored sample reads logical pixel (y, x) of the H x W frame from TRUE
 * column W - 1 - x (the window test applies to the true column: the stored window is not flipped).
 * -> the outputs of kpf_prep_crop_u16 with center = ((u - u0) * d / fx, (v - v0) * d / fy, d) of center_uvd in float (the round trip of the centre, which may
 * differ from it by an ulp, as in the reference), com = center_uvd widened to double, cam_para = cam32; and
 *   joint [B][J][3] float = (xyz - centre) / (float)(cube_z / 2)                                                        (what kpf_eval_errors_f32 takes as gt)
 *   joint_img [B][J][3] float: p = (double)joint * (cube_x / 2) + (double)center in DOUBLE (the reference's cube is an integer array, which promotes), u =
 *       (float)(p_x * fx / p_z + u0), v likewise, d = (float)p_z; crop pixel = (float)(scale * u + m02) (v: m12); then in float u / (S / 2) - 1, v / (S / 2) - 1,
 *       (float)((double)(d - center_z) / (cube_x / 2))
 *   cam64 [B][4] double = cam32 widened: kpf_prep_pcl_sample runs unchanged on img, center, M64, cube and cam64.
 * The intrinsics are used un-mirrored on the mirrored image, as in the reference: a mirrored sample's camera space is the mirrored camera's. */
int kpf_prep_annot_u16(const unsigned char* rgb, const unsigned short* depth, const int* frame_index, int F, const float* joints_mm, const float* cam32,
                       const float* center_xyz, const unsigned char* mirror, const double* cube, int B, int J, int Hs, int Ws, int x0, int y0, int H, int W, int S,
                       float* img, float* img_rgb, float* center, float* M, float* cube_out, float* cam_para, double* com, int* bounds, double* M64, float* joint,
                       float* joint_img, double* cam64, void* stream);

/* kpf_prep_uncrop_mirror_f32 (ABI 23): kpf_prep_uncrop_f32 for the samples of kpf_prep_annot_u16.  mirror [B] bytes, frame_w = W of the logical frame: a
 * mirrored sample's frame_px u is W - 1 - u, taken in double before the rounding to float; crop_px, and every value of an un-mirrored sample, are the bits of
 * kpf_prep_uncrop_f32.  The predicted xyz (joints, crop_px d, frame_px d) stays in the MIRRORED camera's space, as in the reference, which scores left hands
 * there. */
int kpf_prep_uncrop_mirror_f32(const float* joints, const float* center, const float* M, const float* cube, const float* cam, const unsigned char* mirror,
                               int frame_w, int B, int J, float* crop_px, float* frame_px, void* stream);

/* Training augmentation by the dataset protocol (ABI 25): keypointfusion_amd/preprocess.py::prepare_augmented, the reference's TRAINING item
 * (dataloader/loader.py:1140-1156 DexYCB, :1325-1347 HO3D; augmentCrop / augmentCrop_RGB, moveCoM, rotateHand, scaleHand, recropHand, normalize_img).
 *
 * kpf_prep_augment_u16: every argument of kpf_prep_annot_u16 with its meaning, plus per-sample device arrays: mode [B] int (0 rot, 1 com, 2 sc, 3 none:
 * the reference's aug_modes order; any other value is prepared as none), off [B][3] double mm, sc [B] double, rot [B] double degrees, rot_cs [B][2] double =
 * (cos, sin) of fmod(rot, 360) * pi / 180 as the CALLER computed them (no trigonometric function is called here), color [B][3] double or NULL (HO3D's colour
 * scale: clip(value * color, 0, 255) in double before the rounding to float and the / 255).  One workgroup of 1024 threads per sample, grid = B, no
 * allocation, no atomics.  The base crop is kpf_prep_annot_u16's (z-clamped uint16 values in LDS, premax = their maximum); one lane then computes the augmented
 * geometry in double in the host's operation order, one lane per joint the labels, and every thread its destination pixels through the inverse map:
 *   perspective (com, sc): A = Mnew . inv(M), Ai = adj(A) / det(A); W = Ai20 x + Ai21 y + Ai22, W = W != 0 ? 1 / W : 0; X = rint((Ai00 x + (Ai01 y + Ai02)) W),
 *     Y likewise (half to even); affine (rot): the closed-form inverse of getRotationMatrix2D((S/2, S/2), -rot) in OpenCV's 10-bit fixed point: X = (rint((Ai01
 *     y + Ai02) 1024) + 512 + rint(Ai00 x 1024)) >> 10, Y likewise; a source outside [0, S) is the border 0.  (The project's own rule, restated from OpenCV's
 *     nearest-neighbour warps and unpinned against a real OpenCV.)
 * Depth reads the LDS crop, then recropHand's z-threshold in float, normalize_img with the PRE-augmentation maximum and the new centre / cube; RGB reads the
 * frame at the crop pixel's source.  An all-zero depth crop (premax = 0) leaves depth, labels and geometry unaugmented; RGB is warped all the same.
 * -> kpf_prep_annot_u16's outputs (bounds: those of the BASE crop) with center, M, M64, cube_out, com and the labels of the training item, plus cube64 [B][3]
 * double (the cube the sample was normalised with: kpf_prep_pcl_sample takes it in place of cube) and aug_status [B] int: bit 0 = the depth side was
 * augmented, bit 1 = REFUSED parameters (a non-finite off / rot / rot_cs / sc / color, sc <= 0, an offset that takes the centre to where it does not project, a
 * singular map, or new bounds that are degenerate or saturated): the sample is
 * prepared as mode none.  No index is formed from a NaN: every float-to-int conversion saturates and every index is range-tested. */
int kpf_prep_augment_u16(const unsigned char* rgb, const unsigned short* depth, const int* frame_index, int F, const float* joints_mm, const float* cam32,
                         const float* center_xyz, const unsigned char* mirror, const double* cube, const int* mode, const double* off, const double* sc,
                         const double* rot, const double* rot_cs, const double* color, int B, int J, int Hs, int Ws, int x0, int y0, int H, int W, int S,
                         float* img, float* img_rgb, float* center, float* M, float* cube_out, float* cam_para, double* com, int* bounds, double* M64,
                         float* joint, float* joint_img, double* cam64, double* cube64, int* aug_status, void* stream);

/* kpf_prep_aug_draw (ABI 25): the reference's rand_augment (dataloader/loader.py:495-498) and HO3D's colour scale from a counter hash of seed [B] (device,
 * read then advanced: seed[b] += seed_stride, so that a replayed graph draws anew) — preprocess.draw_augment is the host twin, bit-equal except rot_cs.
 * Uniform k of sample b: u = (53 bits of two hash words) * 2^-53, a + (b - a) * u like random.uniform.  mode = floor(4 u0); off = (-1 + 2 u) * sigma_com for
 * u1..u3; rot = -range + (2 range) u4; sc = |1 + (-1 + 2 u5) * sigma_sc|; color = (1 - f) + ((1 + f) - (1 - f)) u for u6..u8; rot_cs = (cos, sin) of fmod(rot,
 * 360) * pi / 180 by the device's double library (within 4 ulp).  Python's Mersenne-Twister stream is not reproduced.  One thread per sample. */
int kpf_prep_aug_draw(long long* seed, int B, double sigma_com, double sigma_sc, double rot_range, double color_factor, long long seed_stride, int* mode,
                      double* off, double* sc, double* rot, double* rot_cs, double* color, void* stream);

/* Device-resident MESH evaluation (ABI 32; keypointfusion_amd/evaluation_mesh_gpu.py, yardstick keypointfusion_amd/evaluation_mesh.py): the figures the
 * HO3D / FreiHAND servers report for a predicted mesh against a ground-truth mesh of the same V vertices.  Device buffers throughout, no entry synchronises or
 * allocates, no floating-point atomics, and the arithmetic below is part of the interface: a sample's bits depend neither on B, nor on its position in the
 * batch, nor on a graph replay.
 *
 * kpf_eval_mesh_f32: pred, gt [B][V][3] float (mm); pred_origin, gt_origin [B][3] float, given together or both NULL (the root-relative protocol: each set minus
 * its origin); thresholds [T] double, f_thresholds [Tf] double (mm).  1 <= V <= 1024, 1 <= T <= 256, 1 <= Tf <= 8, else KPF_EINVAL before the launch and
 * nothing is written.  One 256-thread workgroup per hand; LDS 60 V bytes (both sets as float64, the logged err and nn as float32) + 320.  Leading index 0
 * is the plain pass, 1 the aligned pass over the same buffer; the second index of nn / nn_idx is the direction, 0 pred -> gt, 1 gt -> pred.
 *   All arithmetic in double from the float inputs, every operation individually rounded (no contraction), each result rounded ONCE to float:
 *   a_v = (double)pred_v - (double)pred_origin, g_v = (double)gt_v - (double)gt_origin (no subtraction without origins).
 *   err [2][B][V] float = (float)sqrt(d0*d0 + d1*d1 + d2*d2), d = a_v - g_v, summed left to right.
 *   Every sum over vertices is ONE tree: thread t adds its vertices t, t + 256, ... in ascending order onto +0.0; the 64-lane xor butterfly (offsets 32,
 *   16, .. 1) of each wave; then ((w0 + w1) + w2) + w3 over the four waves.  mean_err [2][B] double = tree sum of (double)err_v, divided by V.
 *   aligned pass: the Umeyama alignment of kpf_eval_errors_f32 over all V vertices: centroids = tree sum / V; H[i][k] = tree sum of a0_i * b0_k, / V;
 *   var = tree sum of (a0_0*a0_0 + a0_1*a0_1 + a0_2*a0_2), / V; rotation R and trace tr of H as there (8 Jacobi sweeps, signed third singular value);
 *   scale = tr / var; a_v <- scale * (R[k][0]*a0_0 + R[k][1]*a0_1 + R[k][2]*a0_2) + centroid(g)_k.  When every predicted vertex is the same point, var and
 *   H are 0 and scale = 0 / 0: the aligned err and mean_err of that sample are NaN, its plain figures and every other sample are unaffected.
 *   nn, nn_idx [2][2][B][V] float / int: for every vertex of one set the nearest vertex of the other: d2 = (dx*dx + dy*dy) + dz*dz over the candidates in
 *   ascending index with a strict <, starting from +inf (the LOWEST index wins a tie; a NaN distance never wins); nn = (float)sqrt(d2min), nn_idx = the
 *   winner, or -1 with nn = +inf when nothing won (the aligned pass of a sample whose alignment is NaN).
 *   pck_cnt [2][B][T] int = number of v with (double)err_v <= thresholds[t]; f_cnt [2][B][Tf][2] int = number of v with (double)nn_v <= f_thresholds[k], last
 *   index the direction: both on the LOGGED floats; NaN and +inf never count. */
int kpf_eval_mesh_f32(const float* pred, const float* gt, const float* pred_origin, const float* gt_origin, const double* thresholds, int T,
                      const double* f_thresholds, int Tf, int B, int V, float* err, float* nn, int* nn_idx, double* mean_err, int* pck_cnt, int* f_cnt,
                      void* stream);

/* kpf_eval_mesh_accumulate: err, mean_err, pck_cnt, f_cnt of the call above; valid NULL or [B] bytes (0 drops a sample).  One workgroup; every state element is
 * owned by one thread that walks the samples b = 0 .. B-1 in ascending order and skips valid == 0; a batch without a valid sample changes nothing:
 *   n_samples [1] += valid samples, n_batches [1] += 1                                                                       (64-bit integers)
 *   sum_mean_err [2] double: x = x + mean_err[a][b];   sum_vert [2][V] double: x = x + (double)err[a][b][v]
 *   pck [2][T] 64-bit integers += pck_cnt[a][b][t]
 *   sum_f [2][Tf][3] double: x = x + (F, P, R) of sample b at f_thresholds[k]: P = f_cnt[..][0] / (double)V, R = f_cnt[..][1] / (double)V,
 *       F = (P + R > 0) ? 2.0 * P * R / (P + R) : 0.0, evaluated left to right. */
int kpf_eval_mesh_accumulate(const float* err, const double* mean_err, const int* pck_cnt, const int* f_cnt, const unsigned char* valid, int B, int V, int T,
                             int Tf, long long* n_samples, long long* n_batches, double* sum_mean_err, double* sum_vert, long long* pck, double* sum_f,
                             void* stream);

/* The result drawn over the frame (ABI 34; keypointfusion_amd/overlay.py, whose draw_host restates both launches in numpy fp32 and gives the same bits;
 * DESIGN.md 4.19).  Device buffers unless marked HOST; no entry synchronises or allocates.  Every floating-point operation is individually rounded fp32
 * (no fma) and every decision that depends on arrival order is an integer min.  Anything outside the stated ranges is refused before the launch with
 * KPF_EINVAL and a kpf_last_error text, and nothing is written.
 *
 * kpf_overlay_project_f32, one workgroup per hand: verts [B][778][3] mm in the camera frame; normals [B][778][3] (kpf_mano_normals_f32's) or NULL;
 * cam [B][4] = fx, fy, u0, v0; M [B][2][3], frame pixels -> target-grid coordinates, or NULL = the identity; sample_offset finite; 0 <= ambient <= 1;
 * 1 <= H, W (the target grid); 1 <= B < 2^20.
 *   U, V, sx, sy, iz are kpf_mano_raster_f32's expressions with sample_offset in place of the literal 0.5: grid pixel (c, r) is sampled at sx = c, sy = r.
 *   sample_offset is 0.5 for a crop grid reached through M (the preprocessing back-projects crop pixel (c, r) from (c + 0.5, r + 0.5)) and 0 for the frame
 *   itself, where the un-crop of a joint (kpf_prep_uncrop_f32's frame_px) is x*fx/z + u0 with no half-pixel shift.
 *   shade = ambient + (1 - ambient) * |n.z|; ambient where the normal is all-zero or not finite; 1 when normals is NULL.
 *   ok = 1 iff x, y, z are finite and z > 0.  rect [B][4] = c0, r0, c1, r1 over the ok vertices (fmin / fmax, a NaN coordinate is skipped):
 *   c0 = min(max(ceil(min sx), 0), W), c1 = max(min(floor(max sx), W - 1), -1), r0 and r1 alike with H, clamped in float before the conversion; a hand
 *   with no ok vertex, or off the grid, has c1 < c0 or r1 < r0. */
int kpf_overlay_project_f32(const float* verts, const float* normals /*or NULL*/, const float* cam, const float* M /*or NULL*/, float sample_offset,
    float ambient, int H, int W, float* sx /*[B][778]*/, float* sy, float* iz, float* shade, int* ok /*[B][778]*/, int* rect /*[B][4]*/, int B,
    void* stream);

/* kpf_overlay_draw_u8, one 256-thread workgroup per 64 x 64 tile of the target grid and stored frame, the tile's 64-bit z-keys in 32 KiB of LDS.
 *   Mesh (sx != NULL; otherwise none is drawn and the mesh's other fields are ignored): every hand b with frame_index[b] (clamped to 0..F-1; NULL: F == B
 * and hand b lies on frame b) equal to the frame, mesh_on NULL or mesh_on[b] != 0, and a rect that meets the tile.  Faces, edge functions, the inside rule
 * and d are kpf_mano_raster_f32's; a face with a vertex that is not ok is dropped; a candidate is a d that is finite and > 0; the smallest
 * (bits(d) << 32) | (hand << 11 | face) wins the pixel: the nearest surface whichever hand it belongs to, among equal d the lowest hand, then the lowest
 * face.  At the winner s = ((w0/sum)*s0 + (w1/sum)*s1) + (w2/sum)*s2 over its vertices' shade.  The pixel is HIDDEN iff depth_frame != NULL, its value
 * o != 0 and (float)o < d - occl_margin: it keeps rgb and gets label 4.  Otherwise channel k is floor(((1 - alpha)*(float)rgb_k + alpha*(mesh_color[hand][k]*s))
 * + 0.5) clamped to 0..255 (NaN -> 0), 1 - alpha computed once in float, and the label is 1.  owner = hand, prim = face, depth = d, hidden or not.
 *   Skeleton (joints_px != NULL), over the mesh, opaque, no depth test: pixel (c, r) is the point ((float)c, (float)r) of joints_px' coordinates, and the
 * LAST covering primitive wins in the order: hands ascending (of this frame, skel_on NULL or skel_on[b] != 0); within a hand joints 0..J-1, then bones
 * 0..NB-1.  A joint (u, v) covers iff u, v are finite, the pixel is inside its box [(u - R) - 1, (u + R) + 1] x [(v - R) - 1, (v + R) + 1] and
 * dx*dx + dy*dy <= R*R with (dx, dy) = pixel - (u, v), R = joint_radius.  A bone a -> b covers iff both ends are finite, the pixel is inside its box
 * [(min(a.x, b.x) - h) - 1, (max(a.x, b.x) + h) + 1] x (y alike), h = bone_half_width, and with e = b - a, p = pixel - a, L = e.x*e.x + e.y*e.y,
 * t = L > 0 ? fmin(fmax((p.x*e.x + p.y*e.y) / L, 0), 1) : 0, q = p - t*e:  q.x*q.x + q.y*q.y <= h*h.  The boxes, one pixel beyond the primitive's
 * extent, are what a tile culls by.  A skeleton pixel gets the primitive's colour, label 3 (joint) or 2 (bone), owner = hand, prim = the joint's or
 * bone's index; depth stays the mesh's.
 *   A pixel nothing covers: out = rgb, label 0, owner = prim = -1, depth 0.
 *   Ranges: 1 <= B < 2^20, 1 <= F <= 65535, 1 <= H, W; 0 <= alpha <= 1; occl_margin finite; with a mesh 1 <= Fc <= 2048 and none of its pointers NULL;
 * with a skeleton 1 <= J <= 64, 0 <= NB <= 64, every bone index in [0, J), joint_radius and bone_half_width finite and >= 0; out must not overlap rgb. */
typedef struct {
  const float *sx, *sy, *iz, *shade;      /* [B][778]: kpf_overlay_project_f32's; sx NULL = no mesh */
  const int *ok, *rect;                   /* [B][778], [B][4]: the same launch's */
  const int* faces;                       /* [Fc][3] */
  const float* mesh_color;                /* [B][3], 0..255 */
  const unsigned char* mesh_on;           /* [B] or NULL */
  const int* frame_index;                 /* [B] or NULL */
  const unsigned char* rgb;               /* [F][H][W][3] */
  const unsigned short* depth_frame;      /* [F][H][W] mm or NULL */
  const float* joints_px;                 /* [B][J][3] = u, v, d in target-grid pixels, or NULL = no skeleton */
  const unsigned char* skel_on;           /* [B] or NULL */
  const int* bones;                       /* HOST [NB][2]: read before the launch and passed with it */
  const unsigned char* bone_color;        /* HOST [NB][3] */
  const unsigned char* joint_color;       /* HOST [J][3] */
  unsigned char* out;                     /* [F][H][W][3] */
  unsigned char* label;                   /* [F][H][W] or NULL: 0 nothing, 1 mesh, 2 bone, 3 joint, 4 mesh hidden by the scene */
  int *owner, *prim;                      /* [F][H][W] or NULL */
  float* depth;                           /* [F][H][W] or NULL: the model depth in mm, 0 where no mesh */
  int B, F, H, W, Fc, J, NB;
  float occl_margin, alpha, joint_radius, bone_half_width;
} kpf_overlay_draw_desc;
int kpf_overlay_draw_u8(const kpf_overlay_draw_desc* d, void* stream);

/* The depth stream registered to the colour camera (ABI 35; keypointfusion_amd/sensor.py, whose align_depth_host restates the rule in numpy fp32 and
 * gives the same bits).  Three launches on the stream -- clear, scatter (one thread per raw pixel), finish (one thread per colour pixel)
 * -- no synchronisation, no allocation; the launches communicate through integer atomics only and each reads what the launch before it completed.
 *   depth_raw [F][Hd][Wd] uint16 raw counts, 0 = no measurement; calib HOST [F][21] float: fxd, fyd, u0d, v0d (the depth camera), fxc, fyc, u0c, v0c (the
 * colour camera), R[9] row-major and t[3] in mm (X_c = R X_d + t), unit_mm (mm per raw count): read before the launch and passed with it; Hc, Wc: the
 * colour grid; zbuf [F][Hc][Wc] uint32 scratch; depth_out [F][Hc][Wc] uint16 mm, 0 = nothing; stats [F][5] int32.
 *   Pixel (c, r) is the point (c, r) and its footprint c +- 0.5, r +- 0.5 (kpf_prep_uncrop_f32's frame pixels, and camera calibrations).  Every
 * floating-point step is one individually rounded fp32 operation (no fma).  Per raw pixel (c, r) of frame f with count q > 0 (stats[f][0] counts them):
 *   1. z = (float)q * unit_mm.
 *   2. carry(pu, pv): X = ((pu - u0d) / fxd) * z, Y = ((pv - v0d) / fyd) * z; Xc = ((R00*X + R01*Y) + R02*z) + t0, Yc and Zc alike from rows 1 and 2;
 *      u = (Xc*fxc) / Zc + u0c, v = (Yc*fyc) / Zc + v0c.
 *   3. a = carry(c - 0.5, r - 0.5), b = carry(c + 0.5, r + 0.5), m = carry(c, r); d = rintf(Zc of m), half to even.
 *   4. The pixel is SKIPPED (stats[f][1]) unless the three Zc are > 0, the nine values u, v, Zc are finite and 1 <= d <= 65535.
 *   5. x0 = ceil(fmin(ua, ub)), x1 = ceil(fmax(ua, ub)) - 1, y0 and y1 alike from v, in float: the colour pixels whose centres lie in [lo, hi) of the box
 *      of the two carried corners.  (An identity calibration covers exactly pixel (c, r) whichever way the last bit of u rounds.)
 *   6. If (x1 - x0) + 1 > max_span or (y1 - y0) + 1 > max_span, in float, the pixel is TOO LARGE (stats[f][2]) and writes nothing: the bound on the work
 *      of a point close to the colour camera's plane.
 *   7. X0 = fmax(x0, 0), X1 = fmin(x1, Wc - 1), Y0 = fmax(y0, 0), Y1 = fmin(y1, Hc - 1), in float; nothing is written unless X0 <= X1 and Y0 <= Y1, and
 *      only then are the four converted to integers.
 *   8. Every zbuf entry of [Y0, Y1] x [X0, X1] takes min(current, (uint32)d): an integer atomic min on a buffer cleared to 0xFFFFFFFF, so the result does
 *      not depend on the order of arrival.
 * Finish: u = (zbuf == 0xFFFFFFFF) ? 0 : zbuf is the unfilled map (stats[f][3] counts its non-zero pixels).  fill = 0: depth_out = u.  fill = 1: a pixel
 * with u == 0 takes the smallest non-zero u of its 4-neighbours if at least two of them are non-zero (stats[f][4] counts these), the neighbours read from
 * the UNFILLED map and counting as 0 outside the grid: the cracks of a resampling are one pixel wide and close, an occlusion shadow stays empty.
 *   Refused before the launch, nothing written: a NULL pointer; F, Hd, Wd, Hc or Wc < 1; F > 32; Hd*Wd or Hc*Wc > 2^24; a calib entry that is not
 * finite; fxd, fyd, fxc, fyc or unit_mm <= 0; max_span outside 1..16; fill not 0 or 1; depth_out overlapping depth_raw. */
int kpf_align_depth_u16(const unsigned short* depth_raw, int Hd, int Wd, const float* calib /*HOST [F][21]*/, int F, int Hc, int Wc, int max_span, int fill,
                        unsigned* zbuf /*[F][Hc][Wc] scratch*/, unsigned short* depth_out /*[F][Hc][Wc]*/, int* stats /*[F][5]*/, void* stream);

/* The hands found in the registered depth frame, and lost tracks seeded from them (ABI 36; keypointfusion_amd/detect.py, whose detect_hands_host and
 * assign_host restate both rules in numpy and give the same words).  The classic depth-camera rule: the hand is the part of the nearest
 * connected surface that reaches towards the camera.
 *   kpf_detect_hands_u16: six launches on the stream for any content -- tiles (union-find in LDS), seams (unions in global memory), flatten + count and
 * z_min, near-slab sums, candidates, selection -- no synchronisation, no readback, no allocation; each launch reads what the one before completed, and
 * only integer atomics (32-bit min, max, add; 64-bit add) touch shared words, so every output is the same bits whatever the order of arrival.
 *   depth [F][H][W] uint16 mm, registered to the camera of cam; cam HOST [F][4] float (fx, fy, u0, v0) of each stored frame's camera, read before the
 * launch and passed with it; K = slots.  Per frame:
 *   1. A pixel is VALID when near <= d <= far, both ends included (stats[f][0] counts them).
 *   2. Two 4-neighbours are JOINED when both are valid and |d_a - d_b| <= step_mm.  Components are the classes of that relation (stats[f][1]); a
 *      component's label is the smallest linear index r * W + c among its pixels: unique, and independent of any order.  Diagonal contact does not join.
 *   3. Per component the pixel count n and z_min.  A component with n < min_pixels is dropped (stats[f][2] counts the others).
 *   4. The NEAR SLAB is the component's pixels with d <= z_min + reach_mm.  In integers: the slab count, S2 = sum d^2, sum u, sum v, sum d (64-bit), and
 *      the inclusive pixel bounds x0, y0, x1, y1.
 *   5. area_mm2 = (double)S2 / ((double)fx * (double)fy): each slab pixel contributes its back-projected area.  A component is a CANDIDATE when
 *      min_area_mm2 <= area_mm2 <= max_area_mm2 (stats[f][3]).
 *   6. Candidates are ranked by (z_min, label) ascending; the first K fill the slots in that order (stats[f][4] = min(candidates, K)), the rest are counted
 *      only.
 *   7. A slot's box is kpf_track_step_f32's rule (tracking.next_bbox) on the two float points (x0, y0), (x1, y1) with frame W, H and `expansion`; where
 *      the rule gives no box the slot is invalid.
 *   boxes [F][K][4] double xywh (0 for an invalid or empty slot), valid [F][K] int, info [F][K][8] double: label, z_min, n, slab count, area_mm2, and the
 * slab centroid u, v, d (the integer sums divided in double); an empty slot holds label -1 and zeros.  labels [F][H][W] int: the component's label, -1 for
 * invalid pixels and for pixels of dropped components.  stats [F][5] int.  ws32: F * 8 * H * W ints of scratch, ws64: kpf_detect_ws64_words(F, H, W, K)
 * 64-bit words (-1: refused).
 *   Limitation: two hands joined through the body inside [near, far] are one component; only the nearer reaches the slots.  Set far to arm's length.
 *   Refused before the launch, nothing written: a NULL pointer; F, H or W < 1; F > 32; H * W > 2^24; K outside 1..8; not 0 <= near <= far <= 65535;
 * step_mm or reach_mm outside 0..65535; min_pixels < 1; an area bound that is not finite, or not 0 <= min <= max; expansion not in (0, 1e6); a cam entry
 * that is not finite; fx or fy <= 0; a pointer not aligned to its element size. */
long kpf_detect_ws64_words(int F, int H, int W, int K);
int kpf_detect_hands_u16(const unsigned short* depth, int F, int H, int W, const float* cam /*HOST [F][4]*/, int near, int far, int step_mm, int reach_mm,
                         int min_pixels, double min_area_mm2, double max_area_mm2, float expansion, int K, int* ws32, long long* ws64,
                         double* boxes /*[F][K][4]*/, int* valid /*[F][K]*/, double* info /*[F][K][8]*/, int* labels /*[F][H][W]*/, int* stats /*[F][5]*/,
                         void* stream);
/* The slots handed to the tracks, one launch (detect.assign_host).  frame_index [B] int: each track's stored frame; the state bbox [B][4] double, lost [B],
 * seeded [B] int is updated in place, reseeded [B] int is rewritten by every call.  A track is FREE when seeded == 0 or lost >= reseed_after, otherwise
 * LIVE.  A valid slot is TAKEN when its slab centroid (u, v) lies inside the box of a live track on the same frame: x <= u < x + w and y <= v < y + h, in
 * double.  The free tracks of a frame, in track order, take the frame's untaken slots in rank order: such a track gets the slot's box, lost = 0,
 * seeded = 1, reseeded = 1.  A free track that gets nothing and has seeded == 0 holds the whole frame (0, 0, frame_w, frame_h), a defined input of the crop.
 * Two live tracks that drift onto one hand are not resolved here.  Refused: a NULL pointer; F outside 1..32; K outside 1..8; B, frame_w, frame_h or
 * reseed_after < 1. */
int kpf_detect_assign_f64(const double* boxes, const int* valid, const double* info, int F, int K, int frame_w, int frame_h, const int* frame_index, int B,
                          int reseed_after, double* bbox, int* lost, int* seeded, int* reseeded, void* stream);

int kpf_conv_num_tile_cfgs(void);

const char* kpf_last_error(void);
/* Library/ABI version, bumped when a signature or the meaning of an argument changes (KPF_ABI_VERSION is what this header
 * describes; the Python binding refuses a library that reports another). */
#define KPF_ABI_VERSION 36
int kpf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
