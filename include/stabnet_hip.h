/* libstabnet_hip.so -- C ABI of the MI355X (gfx950) StabNet hot path.
 *
 * The reference (cxjyxxme/deep-online-video-stabilization, TensorFlow 1.3) has no FFI: its boundary is the
 * TF1 session -- Python op signatures at graph-build time plus a named-tensor contract at run time
 * (SURVEY.md section 8b).  Each entry point below replaces the TF-op cluster behind one of those Python
 * signatures / fetched tensors; the citation names it (file:line in the reference tree).
 *
 * Conventions (all entry points):
 *   - plain pointers to CALLER-OWNED DEVICE memory, NHWC contiguous float32 unless stated; explicit shapes;
 *     `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - never allocates, frees or synchronises; work that needs scratch takes a caller-provided workspace whose
 *     size is queried up front; every call only enqueues kernels on `stream` (hipGraph-capturable);
 *   - returns 0 on success, negative on error (-1 bad argument, -2 launch failure, -3 workspace too small);
 *     the message is available from stabnet_last_error() (thread-local);
 *   - thread-safe per stream.
 */
#ifndef STABNET_HIP_H
#define STABNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* stabnet_last_error(void);
int stabnet_abi_version(void);

/* ---- mesh + multi-grid warp, forward ------------------------------------------------------------------- */

/* get_4_pts(theta, batch_size) -> pts2            s_net_bundle_nobm.py:29-71
 * + get_Hs(pts2) -> Hs                           spatial_transformer3.py:179-198 (get_H/pinv :144-175)
 * theta [N,(gh+1)(gw+1)*2] -> pts2 [N,gh+1,gw+1,2] (vertex = regular grid + offset, clipped to +-1/do_crop_rate),
 * Hs [N,gh,gw,9] (h = inv(A + 1e-4 I) b, last entry 1), pts1 [N,gh,gw,8] (optional, may be NULL): per cell
 * [x_TL,x_TR,x_BL,x_BR,y_TL,y_TR,y_BL,y_BR] (s_net_bundle_nobm.py:65-66). */
int stabnet_get_4_pts(const float* theta, int N, int grid_h, int grid_w, float do_crop_rate,
                      float* pts1, float* pts2, float* Hs, void* stream);

/* transformer(U, theta=pts2) -> (output, black_pix, img=[x_map,y_map])   spatial_transformer3.py:19,218-301,362-365
 * Fetched in deploy as output_img:0, black_pix:0, get_Hs/Hs:0, x_map:0, y_map:0 (deploy_bundle.py:48-56,286).
 * U [N,H,W,C]; pts2 [N,gh+1,gw+1,2]; out [N,H,W,C]; black,x_map,y_map [N,H,W]; Hs [N,gh,gw,9]. */
int stabnet_transformer_fwd(const float* pts2, const float* U, int N, int H, int W, int C, int grid_h, int grid_w,
                            float* out, float* black, float* x_map, float* y_map, float* Hs, void* stream);

/* Fused get_4_pts + transformer: what one deploy frame / training tower runs after the regressor
 * (s_net_bundle_nobm.py:304-307,332).  pts2 may be NULL. */
int stabnet_warp_fwd(const float* theta, const float* U, int N, int H, int W, int C, int grid_h, int grid_w,
                     float do_crop_rate, float* out, float* black, float* x_map, float* y_map, float* Hs,
                     float* pts2, void* stream);

/* _transform3 map stage + _interpolate from given homographies (spatial_transformer3.py:227-295). */
int stabnet_maps_from_hs_fwd(const float* Hs, const float* U, int N, int H, int W, int C, int grid_h, int grid_w,
                             float* out, float* black, float* x_map, float* y_map, void* stream);

/* interpolate(im, x, y, out_size) -> output      spatial_transformer.py:200-281 (used train_bundle_nobm.py:117-118)
 * im [N,H,W,C]; x,y [N,H,W] normalised coordinates; out [N,H,W,C]. */
int stabnet_interp_fwd(const float* im, const float* x, const float* y, int N, int H, int W, int C, float* out,
                       void* stream);

/* ---- regressor building blocks -------------------------------------------------------------------------- */

/* slim conv2d / conv2d_same (+ folded batch_norm + relu on the INPUT, + bias / residual / relu on the output):
 * the op cluster of resnet_v2_50's bottleneck units called at s_net_bundle_nobm.py:252-253.
 * x NHWC [N,H,W,Cin] (Cin % 16 == 0); w OHWI [Cout][KH][KW][Cin]; symmetric zero pad `pad`; y NHWC [N,Ho,Wo,Cout],
 * Ho = (H + 2 pad - KH)/stride + 1.   A-operand prologue (both or neither): a = relu(a*in_scale[c] + in_shift[c]),
 * applied to in-frame pixels only (padding stays 0).  Epilogue: + bias[n] (or NULL), + residual (or NULL; NHWC
 * [N,res_H,res_W,Cout] read at (oy*res_stride, ox*res_stride) -- slim's `subsample` identity shortcut), relu if
 * relu_out.  Arithmetic: exact float32 MFMA, fp32 accumulate.  workspace: stabnet_conv2d_workspace_bytes().
 * Range: input (over the zero-padded frame), output, weights and the residual's own [N,res_H,res_W,Cout] frame each span fewer than 2^30
 * floats (STABNET_ERR_BAD_ARG otherwise). */
size_t stabnet_conv2d_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
/* Tuning hook (tools/autotune.py): force tile (0 128x128, 1 128x64, 2 64x64; < 0 = built-in choice) and split-K. */
void stabnet_conv_tuning_override(int tile, int splitk);
/* Tuning hook (tools/tune_splitk.py): measured split-K of one convolution shape; ring = 1 for prologue-free launches.
 * splitk <= 0 removes the entry, M < 0 clears the table.  Applies to plans made afterwards. */
void stabnet_conv_tuning_table_set(int M, int Cout, int K, int KH, int ring, int splitk);
/* Which measured split-K table plans made AFTERWARDS use: 0 = the exact-f32-MFMA kernels (default), 1 = the packed split kernels
 * (operand mode 4 of stabnet_net_set_bf16_operands: two workgroups per CU, two-way K split inside the workgroup).  Set it around
 * stabnet_net_create() of a plan that will run in mode 4 (stabnet_amd.regressor does). */
void stabnet_conv_tuning_profile(int profile);
int stabnet_conv2d_fwd(const float* x, const float* w_ohwi, const float* bias, const float* in_scale,
                       const float* in_shift, const float* residual, int res_H, int res_W, int res_stride, float* y,
                       int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu_out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Same, with the NEXT layer's folded batch_norm fused behind the sum: y = act((conv + bias + residual)*out_scale[n] +
 * out_shift[n]) (both or neither; NULL = plain epilogue).  This is how the inference plan runs the
 * conv1 -> bn -> relu -> conv2 -> bn -> relu -> conv3 chain of a bottleneck unit (resnet_v2 `bottleneck`, slim). */
int stabnet_conv2d_fwd_ex(const float* x, const float* w_ohwi, const float* bias, const float* in_scale,
                          const float* in_shift, const float* residual, int res_H, int res_W, int res_stride,
                          const float* out_scale, const float* out_shift, float* y, int N, int H, int W, int Cin,
                          int Cout, int KH, int KW, int stride, int pad, int relu_out, void* workspace,
                          size_t workspace_bytes, void* stream);
/* stabnet_conv2d_fwd_ex on the bf16 matrix pipe with float32-level results ("packed split", operand mode 4 of
 * stabnet_net_set_bf16_operands; replaces the same slim conv2d calls, s_net_bundle_nobm.py:252-253): every float32 operand is the
 * exact sum of three bf16 terms, the product is accumulated in float32 from six bf16 x bf16 partial products.  The weights are
 * split once: stabnet_conv_weight_split_image() writes the fragment-major image (stabnet_conv_weight_image_floats() floats, Cin a
 * multiple of 32) the kernel reads; w_ohwi must still be passed (geometries the packed kernel does not take -- Cin % 32 != 0,
 * other tiles -- run stabnet_conv2d_fwd_ex's exact-f32 kernels on it).  splitk > 0 forces the K split (2 with equal halves runs
 * inside the workgroup, others through `workspace` slabs + a reduce launch); 0 = the planned one.  workspace: at least
 * max(stabnet_conv2d_workspace_bytes(), splitk * N*Ho*Wo*Cout * 4).  The image splits every finite weight exactly (|w| >= 2^-110;
 * within 2^-133 below), FLT_MAX included; x must be finite with |x| in [2^-110, 2^127 (2 - 2^-8)) for f32-equal results (same split
 * limits; the run-time split of x does not saturate: a larger finite x gives NaN).  Non-finite inputs give non-finite outputs over
 * their receptive fields, NaN where stabnet_conv2d_fwd_ex gives +-inf (0 behind relu_out, where fwd_ex gives +inf). */
size_t stabnet_conv_weight_image_floats(int Cout, int KH, int KW, int Cin);
int stabnet_conv_weight_split_image(const float* w_ohwi, int Cout, int KH, int KW, int Cin, float* w_img, void* stream);
int stabnet_conv2d_fwd_packed(const float* x, const float* w_ohwi, const float* w_img, const float* bias, const float* in_scale,
                              const float* in_shift, const float* residual, int res_H, int res_W, int res_stride,
                              const float* out_scale, const float* out_shift, float* y, int N, int H, int W, int Cin,
                              int Cout, int KH, int KW, int stride, int pad, int relu_out, int splitk, void* workspace,
                              size_t workspace_bytes, void* stream);
/* stabnet_conv2d_fwd_packed on an input whose pixels lie x_ld floats apart (0 = Cin; else a multiple of 4 >= Cin): Cin columns of a
 * wider buffer, as the inference plan's conv2 layers read conv1's columns of the merged shortcut | conv1 buffer.  Geometries the ring
 * and packed kernels do not take (the register-staged path) need x_ld == Cin.
 * Range: every operand of the launch -- input, output, residual, weights -- must span fewer than 2^30 floats from its pointer, all
 * x_ld / res_ld columns of every pixel counted (the kernels address with 32-bit offsets); refused with STABNET_ERR_BAD_ARG before the
 * pointers are looked at. */
int stabnet_conv2d_fwd_packed_ld(const float* x, int x_ld, const float* w_ohwi, const float* w_img, const float* bias, const float* in_scale,
                                 const float* in_shift, const float* residual, int res_H, int res_W, int res_stride,
                                 const float* out_scale, const float* out_shift, float* y, int N, int H, int W, int Cin,
                                 int Cout, int KH, int KW, int stride, int pad, int relu_out, int splitk, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* The Profiler kind (see stabnet_prof_kind_name) of the conv launch stabnet_conv2d_fwd_packed makes for this geometry, with
 * (prologue != 0) or without in_scale / in_shift: which kernel the call runs.  Host only, no GPU needed; < 0 on a bad geometry. */
int stabnet_conv2d_packed_kind(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int prologue, int splitk);
/* The Profiler kind of the convolution kernel the calling thread launched last (forward operators, back-to-back, dgrad, the conv
 * layers of a plan): the route the launch itself took with its pointers bound.  -1 before the first launch.  Host only. */
int stabnet_conv_last_launch_kind(void);
/* A bottleneck unit's 1x1 conv3 (K1 -> N1 channels, + bias3 + residual) and the next identity unit's 1x1 conv1 (N1 -> N2 channels) as
 * ONE launch (conv_unit_pair_f32_kernel; the tail of one slim bottleneck_v2 unit and the head of the next, s_net_bundle_nobm.py:252-253):
 *   y3 = conv3(x) + bias3 + residual            (written: the next unit's shortcut)
 *   y1 = act(conv1(relu(y3 * pre_scale + pre_shift)) * out_scale + out_shift)      (out_scale / out_shift optional, relu_out the flag)
 * bit-identical to stabnet_conv2d_fwd_packed of the two convolutions one after the other (splitk = 1).  x [N,H,W,K1], residual
 * [N,H,W,N1] with res_ld floats between pixels (0 = N1); w3_img / w1_img = stabnet_conv_weight_split_image of the weights (w3_img may
 * be null for K1 = 64, which multiplies the float32 weights).  K1 a multiple of 64 up to 256 (not 256 with N2 = 64), N1 a multiple
 * of 128, N2 64 or 128, pre_shift behind pre_scale within 4 GiB (one buffer); STABNET_ERR_BAD_ARG otherwise.
 * Range: every operand of the launch -- input, output, residual, weights -- must span fewer than 2^30 floats from its pointer, all
 * x_ld / res_ld columns of every pixel counted (the kernels address with 32-bit offsets); refused with STABNET_ERR_BAD_ARG before the
 * pointers are looked at. */
int stabnet_conv_unit_pair_fwd(const float* x, const float* w3_ohwi, const float* w3_img, const float* bias3, const float* residual, int res_ld,
                               const float* pre_scale, const float* pre_shift, const float* w1_ohwi, const float* w1_img, const float* out_scale,
                               const float* out_shift, float* y3, float* y1, int N, int H, int W, int K1, int N1, int N2, int relu_out, void* stream);
/* The tail of a slim bottleneck_v2 unit as ONE launch (resnet_v2 `bottleneck`, called at s_net_bundle_nobm.py:252-253; what the
 * inference plan runs for the block-1 / block-2 units of a frame): conv2 (3x3, pad 1, stride 1 | 2, C -> C channels, C = 64 | 128,
 * no bias) -> folded batch_norm (mid_scale, mid_shift) + ReLU -> conv3 (1x1, C -> Cout, Cout % C == 0) with conv2d_fwd_ex's
 * epilogue: y = act((conv3 + bias3 + residual) * out_scale + out_shift).  The C-channel intermediate never reaches memory (a
 * workgroup keeps its activated 64-pixel tile in LDS and feeds the 1x1 GEMM from there).  x [N,H,W,C] with x_ld floats between
 * pixels (0 = C); residual read at (oy*res_stride, ox*res_stride) with res_ld floats between pixels (0 = Cout); y [N,Ho,Wo,Cout].
 * No workspace.  STABNET_ERR_BAD_ARG for other geometries (use two stabnet_conv2d_fwd_ex calls).
 * Range: every operand of the launch -- input, output, residual, weights -- must span fewer than 2^30 floats from its pointer, all
 * x_ld / res_ld columns of every pixel counted (the kernels address with 32-bit offsets); refused with STABNET_ERR_BAD_ARG before the
 * pointers are looked at. */
int stabnet_conv3x3_conv1x1_fwd(const float* x, int x_ld, const float* w2_ohwi, const float* mid_scale, const float* mid_shift,
                                const float* w3_ohwi, const float* bias3, const float* residual, int res_H, int res_W,
                                int res_stride, int res_ld, const float* out_scale, const float* out_shift, float* y, int N, int H,
                                int W, int C, int Cout, int stride, int relu_out, void* stream);

/* ---- the regressor as one plan --------------------------------------------------------------------------
 * get_resnet(x_tensor, reuse, is_training=False, x_batch_size) -> theta       s_net_bundle_nobm.py:250-264
 *   = slim resnet_v2_50(global_pool=False, output_stride=32) -> reduce_mean([1,2]) -> fully_connected 2048/1024/512
 *     -> output_layer (resnet.py:44-56).  The run-time feed/fetch it serves: x_tensor:0 -> (theta ->) the tensors of
 *     deploy_bundle.py:48-56,286.
 * A net handle is a HOST-ONLY description (layer list, buffer offsets); it owns no device memory.
 * Parameter buffer (floats): [weights/biases in network order][BN gammas][BN betas] | [moving means][moving vars];
 * the first stabnet_net_trainable_floats() floats are the trainables.  Conv weights are OHWI with Cin padded to 16,
 * FC weights [out][in]; stabnet_net_param_info() gives name (TF variable name under stable_net/resnet/), offset,
 * kind (0 conv w, 1 conv bias, 2 gamma, 3 beta, 4 moving_mean, 5 moving_variance, 6 FC w, 7 FC bias), dims, aux
 * (conv: un-padded Cin).
 * Range: stabnet_net_create() refuses (STABNET_ERR_BAD_ARG, the message names the layer, the operand and its extent) a shape in which any
 * convolution's input, output, residual or weights would span 2^30 floats or more from its pointer, all x_ld / res_ld columns of the
 * merged buffers counted -- the range the conv kernels address with 32-bit offsets, in every operand mode and fusion, forward and backward. */
int stabnet_net_create(void** net, int N, int H, int W, int in_ch, int n_theta, int keep_activations);
void stabnet_net_destroy(void* net);
/* Conv operand mode of the inference forward (tensors are float32 in memory and accumulation is float32 in every mode):
 *   0  exact f32 MFMA (v_mfma_f32_32x32x2_f32), the default;
 *   1  SECONDARY reduced-precision mode (never the headline): operands rounded to bf16 at fragment-read
 *      time.  Own, looser parity bar (3e-3 on theta);
 *   2 / 3  split operands: every f32 operand is decomposed EXACTLY into three bf16 terms (x = h + m + l) when its fragment is read
 *      and the f32 product is accumulated as six (3: all nine) bf16 x bf16 partial products on v_mfma_f32_32x32x16_bf16 -- f32-level
 *      results (theta within 2e-7 of the oracle, like mode 0) on the 16x faster matrix pipe; VALU-bound, slower than mode 0: kept
 *      as the reference form of mode 4;
 *   4  packed split: the weights are split once into a fragment-major image inside `fold` (stabnet_net_fold_bn), only the A
 *      fragments are split at run time (conv_ring_f32_kernel<MODE, 4, KG, PRO>).  Same f32-level parity bar as mode 0.
 *      Range: mode 4 equals f32 for finite weights of any magnitude (the image's head saturates at the largest finite bf16) and for
 *      finite activations of magnitude in [2^-110, 2^127 (2 - 2^-8)); both splits are exact down to 2^-110 and within 2^-133 (absolute)
 *      below it, and the run-time split of the activations does not saturate: a larger finite activation gives NaN (out of contract).
 *      Non-finite operands give non-finite outputs, but NaN where f32 gives +-inf, and a ReLU epilogue turns that NaN into 0 (fmaxf).
 *   S_CONV_B2B units of a plan (STABNET_CONV_B2B_PLAN=1) run the fused exact-f32 kernel in modes 0 and 4, two launches in modes 1 - 3.
 * Training plans (keep_activations = 1) accept 0 and 4 only; 4 = the step's weight-operand launches (the prologue-carrying 1x1
 * forward pairs, the stride-1 dgrad launches) read images of the forward weights and of the re-packed dgrad weights that the step
 * writes itself, inside its workspace -- call it BEFORE stabnet_net_train_workspace_bytes().  Off by default in the Python
 * mirror (no sustained gain at 8 pairs per GPU on a power-limited part; it pays at larger batches). */
int stabnet_net_set_bf16_operands(void* net, int on);
/* Inference plans in operand mode 4: on != 0 replaces every eligible [conv3, next unit's conv1] pair of plan steps by ONE step (kind 6,
 * conv_unit_pair_f32_kernel): conv3 still writes its output (the next residual), conv1 takes its operand from conv3's accumulators
 * instead of reading that output back.  Bit-identical to the two launches.  A pair is eligible when both are 1x1 / stride 1 / pad 0
 * without a K split, conv3 has no consumer BN, a residual of stride 1 and K <= 256, conv1 is the very next step, reads exactly
 * conv3's output through its prologue and has 64 or 128 output channels, M >= 12288 (STABNET_CONV_PAIR_MIN_M lowers it for tests),
 * conv_route() sends the two launches to the kernels whose arithmetic the fused kernel repeats, and conv1's output overlaps neither
 * conv3's residual nor its input (other than in place).  on == 0 restores the plan as built; so does a later
 * stabnet_net_set_bf16_operands().  In any other mode, on a training plan, or with STABNET_CONV_PAIR=0 the plan stays what it is.
 * Workspace, fold buffer and tensor offsets never change.  Returns 0. */
int stabnet_net_fuse_unit_pairs(void* net, int on);
int stabnet_net_num_params(const void* net);
int stabnet_net_param_info(const void* net, int idx, char* name, int name_cap, long* offset, int* kind, int* dims4,
                           int* aux);
size_t stabnet_net_param_floats(const void* net);
size_t stabnet_net_trainable_floats(const void* net);
size_t stabnet_net_bn_channels(const void* net);
size_t stabnet_net_workspace_bytes(const void* net);
double stabnet_net_flops(const void* net);
int stabnet_net_num_launches(const void* net);
/* Kernel launches of one stabnet_deploy_frame pass (refine = 1) on the CURRENT device: stack assembly + the regressor's
 * launches + (mesh, unless it rides with the output layer's launch: batch <= 8) + sampler-with-push; -1 on a null plan. */
int stabnet_deploy_frame_launches(const void* net, int grid_h, int grid_w);
int stabnet_net_activation_info(const void* net, const char* name, long* offset, int* dims4);

/* slim batch_norm(is_training=False) folded to per-channel (scale, shift): fold = [G scales][G shifts],
 * G = stabnet_net_bn_channels().  scale = rsqrt(var + eps) * gamma, shift = beta - mean * scale. */
int stabnet_net_fold_bn(const void* net, const float* params, float* fold, float eps, void* stream);
/* Floats the caller must allocate for `fold`: 2*bn_channels, plus the re-laid-out stem weights of an inference plan
 * (keep_activations = 0), which reads the 13-channel stack directly (no channel padding). */
size_t stabnet_net_fold_floats(const void* net);

/* x_tensor NHWC [N,H,W,in_ch] -> theta [N,n_theta]; BN in moving-average mode (s_net_bundle_nobm.py:302). */
int stabnet_backbone_fwd_infer(const void* net, const float* params, const float* fold, const float* x_tensor,
                               float* theta, void* workspace, size_t workspace_bytes, void* stream, void* prof);

/* ---- inference plans, one step at a time (keep_activations = 0 only) -------------------------------------------
 * A plan is a list of steps: 0 pad / embed the input, 1 convolution, 2 max-pool, 3 global pool, 4 fully connected, 5 conv2 -> conv3
 * as one launch (STABNET_CONV_B2B_PLAN=1 plans), 6 conv3 -> the next unit's conv1 as one launch (stabnet_net_fuse_unit_pairs; the fields
 * describe the conv3 half as its own launch would be routed, PROF_KIND / TILES .. GZ / LDS_* the fused launch).  Kinds 5 and 6 each stand
 * for two consecutive convolution steps of the plan as built, which is made of kinds 0 - 4 only.
 * stabnet_net_step_info() says what a step is and, for a convolution (kind 1),
 * everything its launch is made of, as the forward would bind and route it in the plan's operand mode (stabnet_net_set_bf16_operands)
 * on a chip of `cus` CUs.  HOST ONLY: no GPU is needed and the device is not read -- `cus` is the caller's (an MI355X has 256).
 * info[STABNET_SI_*], `cap` >= STABNET_SI_FIELDS (= stabnet_net_step_info_fields()) longs; every field of a non-conv step but KIND is 0:
 *   geometry      N H W CIN HO WO COUT KH KW STRIDE PAD, X_LD / RES_LD (floats between pixels of the input / residual), RES_H RES_W
 *                 RES_STRIDE, ROWRUN (the stem's row-run operand), RELU_OUT (the flag as bound), M = N*HO*WO, K
 *   workspace     float offsets: IN_OFF (first float read), IN_BASE / IN_FLOATS (the whole buffer the input lives in: all X_LD columns,
 *                 the row-run stem's border and slack row), OUT_OFF / OUT_FLOATS, RES_OFF (-1: none) / RES_FLOATS (whole buffer, all
 *                 RES_LD columns), SCRATCH_OFF (the split-K slabs start here) / SCRATCH_FLOATS (splitk * M * COUT when a reduce launch
 *                 follows, else 0)
 *   params        float offsets into `params`: W_OFF (OHWI weights), BIAS_OFF (-1: none)
 *   fold          PRO_BN_OFF / OUT_BN_OFF: channel offset c of the input prologue / the consumer's BN + ReLU (scale fold[c ..], shift
 *                 fold[bn_channels + c ..]; -1: none); MERGED_OFF: float offset of the [bias | scale | shift | floor][COUT] vectors
 *                 of a merged shortcut | conv1 launch (they REPLACE bias, output BN and the ReLU flag; -1: none); W_ROWRUN_OFF: the
 *                 row-run copy of the stem's weights (-1: not row-run); W_IMAGE_OFF: the pre-split weight image the launch comes with
 *                 (-1: none)
 *   flags         INF_PREACTIVATED (the input already holds relu(bn(.))), PROLOGUE (the launch applies BN + ReLU to its input)
 *   K split       SPLITK, STEPS_PER_SPLIT, TOTAL_STEPS (K-steps of the whole reduction)
 *   route         conv_route()'s answer for the bound launch: FAMILY (0 register-staged, 1 ring, 2 ring with K groups, 3 ring with
 *                 prologue, 4 packed, 5 packed with two K groups, 6 A-stationary, 7 patch-stationary), MODE, OPERAND, KG, PRO, NBUF, BK,
 *                 TILE, ASTAT_BM, PATCH_CFG, REDUCE (a split-K reduce launch follows), PROF_KIND (stabnet_prof_kind_name)
 *   grid          TILES and WGS = GX * GY * GZ workgroups by the launchers' own rule: (M tile, N tile, K slice) of the 64 x 64 kernels,
 *                 (M tile | patch, pass over the column blocks a workgroup's waves take side by side) of the A-stationary and patch kernels
 *   index math    DIV_HW_MUL / _SHIFT, DIV_W_MUL / _SHIFT: the multiply-high constants the kernels divide by HO*WO and WO with
 *   LDS           LDS_BYTES / LDS_LIMIT: the A-stationary kernel's planes, the patch kernel's launch, and what the launcher holds them to
 * stabnet_net_run_steps() enqueues steps first..last of stabnet_backbone_fwd_infer on the caller's workspace, bound and launched by the
 * forward's own code, and nothing else (the fused head's last launch belongs to the last step).  x_tensor / theta may be NULL when no
 * step of the range reads / writes them.  Returns an error and launches nothing for a training plan, a bad range or a workspace
 * smaller than stabnet_net_workspace_bytes(). */
enum {
    STABNET_SI_KIND = 0,
    STABNET_SI_N, STABNET_SI_H, STABNET_SI_W, STABNET_SI_CIN, STABNET_SI_HO, STABNET_SI_WO, STABNET_SI_COUT, STABNET_SI_KH, STABNET_SI_KW,
    STABNET_SI_STRIDE, STABNET_SI_PAD, STABNET_SI_X_LD, STABNET_SI_RES_LD, STABNET_SI_RES_H, STABNET_SI_RES_W, STABNET_SI_RES_STRIDE,
    STABNET_SI_ROWRUN, STABNET_SI_RELU_OUT, STABNET_SI_M, STABNET_SI_K,
    STABNET_SI_IN_OFF, STABNET_SI_IN_BASE, STABNET_SI_IN_FLOATS, STABNET_SI_OUT_OFF, STABNET_SI_OUT_FLOATS, STABNET_SI_RES_OFF,
    STABNET_SI_RES_FLOATS, STABNET_SI_SCRATCH_OFF, STABNET_SI_SCRATCH_FLOATS,
    STABNET_SI_W_OFF, STABNET_SI_BIAS_OFF, STABNET_SI_PRO_BN_OFF, STABNET_SI_OUT_BN_OFF, STABNET_SI_MERGED_OFF, STABNET_SI_W_ROWRUN_OFF,
    STABNET_SI_W_IMAGE_OFF, STABNET_SI_INF_PREACTIVATED, STABNET_SI_PROLOGUE,
    STABNET_SI_SPLITK, STABNET_SI_STEPS_PER_SPLIT, STABNET_SI_TOTAL_STEPS,
    STABNET_SI_FAMILY, STABNET_SI_MODE, STABNET_SI_OPERAND, STABNET_SI_KG, STABNET_SI_PRO, STABNET_SI_NBUF, STABNET_SI_BK, STABNET_SI_TILE,
    STABNET_SI_ASTAT_BM, STABNET_SI_PATCH_CFG, STABNET_SI_REDUCE, STABNET_SI_PROF_KIND,
    STABNET_SI_TILES, STABNET_SI_WGS, STABNET_SI_GX, STABNET_SI_GY, STABNET_SI_GZ,
    STABNET_SI_DIV_HW_MUL, STABNET_SI_DIV_HW_SHIFT, STABNET_SI_DIV_W_MUL, STABNET_SI_DIV_W_SHIFT,
    STABNET_SI_LDS_BYTES, STABNET_SI_LDS_LIMIT,
    STABNET_SI_FIELDS
};
int stabnet_net_num_steps(const void* net);
int stabnet_net_step_info_fields(void);
int stabnet_net_step_info(const void* net, int step, int cus, long* info, int cap);
int stabnet_net_run_steps(const void* net, const float* params, const float* fold, const float* x_tensor, float* theta,
                          void* workspace, size_t workspace_bytes, int first, int last, void* stream);

/* ---- inference: the non-convolution layers and the head of the plan, one entry per operator -----------------
 * The launchers that stabnet_backbone_fwd_infer / stabnet_deploy_frame / stabnet_net_fold_bn run, reachable one at a time.
 * The plan hands them shapes it laid out itself; these entries refuse (STABNET_ERR_BAD_ARG, nothing launched) what the
 * kernels cannot do: null or host pointers, a pointer the kernel reads as float4 that is not 16-byte aligned, and the shape
 * limits named per entry.  Every sum is taken in a fixed order: the same call gives the same bits. */

/* x_tensor [npix][C] -> y [npix][Cp], zeros in channels C..Cp (the 13 -> 16 channel stack in front of the stem conv,
 * s_net_bundle_nobm.py:252).  Cp % 4 == 0, Cp >= C; y 16-byte aligned. */
int stabnet_pad_channels(const float* x, float* y, long npix, int C, int Cp, void* stream);

/* resnet_v2 `conv1` weights OHWI [Cout][KH][KW][CinPad] -> filter-row runs [Cout][KH][Rp], Rp = roundup(KW*Cin, 32): element
 * kw*Cin + c, zeros behind (the inference stem reads the unpadded Cin-channel stack). */
int stabnet_stem_repack(const float* w, float* out, int Cout, int KH, int KW, int CinPad, int Cin, void* stream);

/* Epilogue vectors of a merged (projection shortcut | conv1) launch of resnet_v2 `bottleneck`: out [4][depth + dbn] =
 * [bias | scale | shift | floor]; shortcut channels (b_sc, 1, 0, -inf), conv1 channels (0, scale1, shift1, 0 = ReLU). */
int stabnet_merge_vectors(const float* b_sc, const float* scale1, const float* shift1, int depth, int dbn, float* out, void* stream);

/* tf.nn.batch_normalization with moving averages, folded: scale = (1 / sqrt(var + eps)) * gamma, shift = beta - mean * scale,
 * each operation one correctly rounded float32 operation (what stabnet_net_fold_bn runs over all G channels). */
int stabnet_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int G, float* scale,
                    float* shift, void* stream);

/* slim max_pool2d [3,3] stride 2 of resnet_v2 ('pool1'), inference form: y [N,Ho,Wo,C] = max over the in-image taps of the
 * window at (oy*stride - pt, ox*stride - pl) (out-of-image taps count as -inf); scale, shift [C] (both or neither): the
 * consumer's folded BN + ReLU on the pooled value, y = max(fma(y, scale, shift), 0).  C % 4 == 0, fewer than 2^32 channel
 * quads N*Ho*Wo*C/4; x, y, scale, shift 16-byte aligned. */
int stabnet_max_pool_fwd(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, int k, int stride, int pt, int pl,
                         const float* scale, const float* shift, void* stream);

/* postnorm batch_norm + relu + tf.reduce_mean(resnet, [1, 2]) (s_net_bundle_nobm.py:254): out [N][C] = mean over HW of
 * max(fma(x, scale, shift), 0), x [N][HW][C].  Sum order: rows r, r+16, ... of a chunk per lane, the 16 lanes, then the
 * chunks (min(32, max(1, HW/32)) of ceil(HW/chunks) rows), one division.  partial: stabnet_gap_partial_floats(N, HW, C)
 * floats of scratch (0 = bad arguments).  C % 4 == 0, N <= 65535; x, scale, shift, partial 16-byte aligned. */
size_t stabnet_gap_partial_floats(int N, int HW, int C);
int stabnet_gap_bn_relu(const float* x, const float* scale, const float* shift, int N, int HW, int C, float* out, float* partial,
                        size_t partial_floats, void* stream);

/* slim.fully_connected / output_layer (s_net_bundle_nobm.py:256-259, resnet.py:44-56): y [M][Nout] = act(x [M][K] w[Nout][K]^T
 * + b), b may be NULL, relu = 0 | 1.  Per output element the same products in the same order whatever M (rows are staged
 * in LDS for 9..16 rows of at most 128 KiB, else read in passes of 16 and 8).  K % 4 == 0; x, w 16-byte aligned. */
int stabnet_fc_fwd(const float* x, const float* w, const float* b, float* y, int M, int K, int Nout, int relu, void* stream);

/* The shortened inference head (batch <= 8).  stabnet_head_fused_supported: 1 when the plan takes it for fc_dims =
 * [C, 2048, 1024, 512, n_theta] (host ints).
 * stabnet_head_gap_fc1: the pooling above as partial sums over min(max(1, 8/N), max(1, HW/16)) chunks, then fc_1 (ReLU) whose
 * input staging adds the chunks and divides by HW: y [N][Nout]; gap_out [N][C] (optional, NULL) receives the pooled feature
 * ("global_pool").  y has the bits of stabnet_fc_fwd(gap_out, relu = 1).  N <= 8, C % 64 == 0, C <= 2048; partial:
 * stabnet_head_gap_partial_floats(N, HW, C) floats (0 = bad arguments).
 * stabnet_head_theta_mesh: output_layer (no activation) theta [N][n_theta] = x [N][K] w[n_theta][K]^T + b, K == 512,
 * n_theta <= 64; Hs (optional, NULL) [N][gh*gw][9]: get_4_pts + get_Hs of that theta (s_net_bundle_nobm.py:29-71), the bits of
 * stabnet_get_4_pts on it -- needs n_theta == 2(gh+1)(gw+1), gh*gw <= 64; head_adv (optional, NULL): *head_adv =
 * (*head_adv + 1) % depth, once per call (the online loop's ring head); prefetch_src (optional, NULL) [N][pf_H][pf_W]: a frame
 * that extra workgroups only read (cache warm-up for the sampler behind; silently off when pf_W % 4 != 0, pf_H < 8 or the
 * pointer is not 16-byte aligned). */
int stabnet_head_fused_supported(int N, int C, const int* fc_dims);
size_t stabnet_head_gap_partial_floats(int N, int HW, int C);
int stabnet_head_gap_fc1(const float* x, const float* scale, const float* shift, int N, int HW, int C, float* partial,
                         size_t partial_floats, float* gap_out, const float* w, const float* b, float* y, int Nout, void* stream);
int stabnet_head_theta_mesh(const float* x, const float* w, const float* b, int N, int K, int n_theta, float* theta, int grid_h,
                            int grid_w, float do_crop_rate, float* Hs, int* head_adv, int depth, const float* prefetch_src, int pf_H,
                            int pf_W, void* stream);

/* ---- the online loop (deploy_bundle.py) ------------------------------------------------------------------ */

/* History ring initialisation: `depth` copies of the first frame and zero masks per stream
 * (deploy_bundle.py:216-224).  frames_ring, masks_ring: [S][depth][H*W]; first_frame [S][H*W]. */
int stabnet_ring_init(float* frames_ring, float* masks_ring, const float* first_frame, int S, int depth, int H, int W,
                      void* stream);

/* One iteration of the hot loop for S = net.N independent streams (deploy_bundle.py:259-296,319-332), the work of
 * one sess.run([output, black_pix, Hs, x_map, y_map], {x_tensor: in_x}) plus the NumPy stack assembly before it and
 * the feedback after it:  13-channel stack from the ring at the dilated `lags` (HOST int array, e.g. 1,2,4,8,16,32;
 * channel order masks, frames, current) -> regressor -> get_4_pts -> transformer -> frame = img - black ->
 * frames_ring[head] = frame, masks_ring[head] = black.  refine > 1 repeats the network on the refined frame
 * (:284-295).  `head` is a DEVICE int[2] = {ring slot of this frame's push, reserved (zero)}; the call
 * advances head[0] to (head+1) % depth on the device (refine = 1: by one thread of the mesh kernel, which sits between
 * the last reader of the head -- the stack assembly -- and the sampler, whose fused feedback push then writes slot
 * head - 1; else by a one-thread kernel at the end), so every argument is fixed across frames
 * and the call can be captured into a hipGraph once and replayed (copy the new frame into the fixed `cur_frame` buffer
 * before each replay).  all_black (optional, may be NULL): int32 [S,H,W] += round(black) once per refine pass
 * (deploy_bundle.py:291, inside the refine loop) -- the input of stabnet_crop_search.
 * Outputs: theta [S,n_theta]; out_img, black, x_map, y_map, frame_fb [S,H,W]; Hs [S,gh,gw,9]. */
int stabnet_deploy_frame(const void* net, const float* params, const float* fold, float* frames_ring,
                         float* masks_ring, int depth, int* head, const int* lags, int n_lags, const float* cur_frame,
                         int refine, int grid_h, int grid_w, float do_crop_rate, float* theta, float* out_img,
                         float* black, float* x_map, float* y_map, float* Hs, float* frame_fb, int* all_black,
                         void* workspace, size_t workspace_bytes, void* stream, void* prof);

/* ---- optional per-launch timing (bench.py roofline leg) --------------------------------------------------
 * A profiler handle owns HIP events (host objects).  Passing it as `prof` to a forward makes that call record an
 * event pair around each kernel launch; read the records after synchronising the stream.  NULL = no instrumentation. */
int stabnet_prof_create(void** prof, int max_records);
void stabnet_prof_destroy(void* prof);
int stabnet_prof_reset(void* prof);
int stabnet_prof_record_empty(void* prof, void* stream);   /* an event pair around nothing: the overhead to subtract */
int stabnet_prof_num_records(const void* prof);
int stabnet_prof_record(const void* prof, int idx, int* kind, float* ms, double* flops, double* bytes);
int stabnet_prof_record_shape(const void* prof, int idx, int* shape4);
const char* stabnet_prof_kind_name(int kind);

/* ---- measurement helpers (bench.py: empirical peaks of the box beside the vendor peaks; not on the path) ---- */
int stabnet_probe_mfma_f32(float* out /* blocks*256 floats */, int blocks, int iters,
                           unsigned long long* stamps /* optional, device [blocks][2]: {shader cycles, 100 MHz ticks} in the loop */,
                           void* stream);
double stabnet_probe_mfma_f32_flops(int blocks, int iters);
int stabnet_probe_hbm_copy(const float* src, float* dst, long n_floats, void* stream);
/* Stand-in for a collective's kernel on a one-GPU box: dst[i] += src[i] by `workgroups` long-lived
 * workgroups of 256 threads holding lds_bytes (<= 64 KiB) of LDS each; stamps (optional, device, 2 words per workgroup):
 * 100 MHz ticks at its entry and exit.  Not on the product path. */
int stabnet_probe_comm_proxy(const float* src, float* dst, long n_floats, int workgroups, int lds_bytes, unsigned long long* stamps,
                             void* stream);
/* CUs the persistent convolution kernels leave free (0 = none, the default): their grids are sized for (CUs - reserved) x
 * workgroups-per-CU, so that a collective's kernel on a communication stream finds CU slots without waiting for a kernel
 * boundary.  Never fewer than an eighth of the chip stays usable: the grids are sized for max(CUs / 8, CUs - reserved) CUs, so any
 * reserved >= CUs - CUs / 8 behaves alike; a negative value stores 0.  The setting moves tiles between workgroups only: results are
 * bit-identical for every value.  A process-wide setting read at launch time (train.Trainer sets it from STABNET_COMM_RESERVED_CUS
 * when it has a process group); returns the previous value. */
int stabnet_conv_reserve_cus(int reserved);

/* ---- training: backward of the warp / sampler and the loss kernels ---------------------------------------
 * These replace what TF autodiff generates for `opt.minimize(total_loss)` (train_bundle_nobm.py:160) over the ops
 * above.  floor / casts / comparisons carry no gradient (corners, black_pix, z sign, warp_pts indices are constants). */

/* Reproducibility: every reduction below is order-independent (64-bit fixed-point accumulation, scale 2^40, or block
 * partials added in a fixed order) -- two runs of a training step on the same inputs give the same bits.
 *
 * d transformer / d pts2 (pre-clip vertex gradient) [N,gh+1,gw+1,2] from d_out [N,H,W,C], d_xmap, d_ymap [N,H,W]
 * (each may be NULL); dmap_scale [N] (optional) multiplies d_xmap / d_ymap per sample (stabnet_feature_loss hands over
 * signed counts and that factor).  x_map, y_map, Hs: the forward's outputs.  workspace: N*gh*gw*8 + 1 8-byte words (8-B aligned).
 * A non-finite or out-of-range (|v| >= 2^22) contribution poisons the sums: the gradients then come out NaN, not finite garbage. */
int stabnet_transformer_bwd(const float* pts2, const float* Hs, const float* U, const float* x_map, const float* y_map,
                            const float* d_out, const float* d_xmap, const float* d_ymap, const float* dmap_scale, int N,
                            int H, int W, int C, int grid_h, int grid_w, float* d_pts2, void* workspace, void* stream);

/* d interpolate(im, x, y) / d im  (train_bundle_nobm.py:117-118): scatter-add of the four taps, d_im (+)= it.
 * workspace: N*H*W*C + 1 8-byte words (8-B aligned); non-finite contributions give NaN (see stabnet_transformer_bwd). */
int stabnet_interp_bwd(const float* x, const float* y, const float* d_out, int N, int H, int W, int C, float* d_im,
                       int accumulate, void* workspace, void* stream);

/* Re-packing helpers of the host mirror: out [npix] = x[npix][C][:, c] (x_tensor[..., 12:13] of s_net_bundle_nobm.py:281,
 * flow[..., 0]); out [n][2] = (a, b) interleaved (img = [x_map, y_map], spatial_transformer3.py:295). */
int stabnet_slice_channel(const float* x, long npix, int C, int c, float* out, void* stream);
int stabnet_interleave2(const float* a, const float* b, long n, float* out, void* stream);

/* y = a*x + b elementwise (1 - black_pix of train_bundle_nobm.py:118). */
int stabnet_axpb(const float* x, float a, float b, long n, float* y, void* stream);

/* masked MSE of img_loss (s_net_bundle_nobm.py:347-352, m2 = NULL) and temp_loss (train_bundle_nobm.py:110-125,
 * m2 = interp(1 - black2)): sums [N,2] = {sum((a-b)m)^2, sum m}, m = (1 - black) * m2;
 * loss = sum_n sums[n][0] / (sums[n][1] + 1e-8) / batch_size.  _grad: ga (+)= coef * dloss_unnormalised/da, gb = -that. */
size_t stabnet_masked_mse_workspace_bytes(int N);
int stabnet_masked_mse_sums(const float* a, const float* b, const float* black, const float* m2, int N, long hw,
                            float* sums, void* workspace, void* stream);
int stabnet_masked_mse_grad(const float* a, const float* b, const float* black, const float* m2, const float* sums,
                            float coef, int N, long hw, float* ga, int accumulate_a, float* gb, void* stream);

/* feature loss (s_net_bundle_nobm.py:215-230,335-343): value [N] = masked mean L1 between the maps gathered at the
 * rounded stable point and the unstable point; its gradient wrt the maps = d_xmap / d_ymap (signed counts +-mask scattered
 * at the rounded pixels; zeroed here; both NULL = forward only) times dscale [N] = gcoef / max(sum mask, 1);
 * warped [N,max_matches,2] optional (ret['stable_warpped']). */
int stabnet_feature_loss(const float* matches, const float* mask, const float* x_map, const float* y_map, int N, int H,
                         int W, int max_matches, float gcoef, float* value, float* d_xmap, float* d_ymap, float* dscale,
                         float* warped, void* stream);

/* losses4 = {id2_loss (= mean|theta| * id_mul, :263), black_pos mean (:139-146,312-317), distortion (:148-181),
 * consistency (:183-210)}; d_theta [N,n_theta] = clip-mask (:58) * (d_pts2_warp + w_dist d dist + w_cons d cons +
 * w_black d black) + w_id * d id2_loss (d_theta may be NULL: values only). */
int stabnet_mesh_losses(const float* theta, const float* d_pts2_warp, int N, int grid_h, int grid_w, float do_crop_rate,
                        float id_mul, float w_id, float w_dist, float w_cons, float use_black, float w_black,
                        float* losses4, float* d_theta, void* stream);

/* ---- training: convolution backward (autodiff of slim conv2d) --------------------------------------------- */

/* dW (OHWI, ACCUMULATED into, not zeroed) += d conv2d / d weights.  x: forward input; (in_scale,in_shift): the forward's
 * folded-BN + ReLU prologue (both or NULL); dy [N,Ho,Wo,Cout].  Exact float32 MFMA; the pixel range is split over
 * workgroups whose partial tiles go to slabs in `workspace` and are added in split order (reproducible, no atomics).
 * dw (and d_bias below) must be 16-byte aligned: the slab reduction updates them 16 B at a time (STABNET_ERR_BAD_ARG otherwise). */
size_t stabnet_conv2d_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int stabnet_conv2d_wgrad(const float* x, const float* dy, float* dw, const float* in_scale, const float* in_shift,
                         int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, void* workspace,
                         size_t workspace_bytes, void* stream);

/* 1x1 stride-1 layers with Cout % 256 == 0: dW as above and d_bias [Cout] += column sums of dy from the same pass over dy
 * (what the training step does for the unit-closing convolutions).  Other geometries: STABNET_ERR_BAD_ARG. */
size_t stabnet_conv2d_wgrad_bias_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int stabnet_conv2d_wgrad_bias(const float* x, const float* dy, float* dw, float* d_bias, const float* in_scale, const float* in_shift,
                              int N, int H, int W, int Cin, int Cout, void* workspace, size_t workspace_bytes, void* stream);

/* The same for a channel count that is not a multiple of 4 (the 13-channel stem input): x [N,H,W,Cin] tight,
 * dw OHWI [Cout][KH][KW][CinPad] accumulated into (pad channels untouched).  x is embedded in a zero-bordered image inside
 * `workspace` and read as runs of KW*Cin contiguous floats per filter row -- the operand layout of the training step's stem. */
size_t stabnet_conv2d_wgrad_rowrun_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int stabnet_conv2d_wgrad_rowrun(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int CinPad, int Cout,
                                int KH, int KW, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);

/* dx [N,H,W,Cin] = d conv2d / d input (+ residual if given, may alias dx) from dy [N,Ho,Wo,Cout] and the forward
 * weights (OHWI).  Cout % 16 == 0.  workspace: stabnet_conv2d_dgrad_workspace_bytes() (re-packed weights + split-K). */
size_t stabnet_conv2d_dgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int stabnet_conv2d_dgrad(const float* dy, const float* w_ohwi, float* dx, const float* residual, int N, int H, int W,
                         int Cin, int Cout, int KH, int KW, int stride, int pad, void* workspace,
                         size_t workspace_bytes, void* stream);

/* The forms of the above that a backward stage of the training step runs, on the step's own launchers (operator tests).
 *
 * stabnet_conv2d_wgrad_layers: the weight gradients of L >= 1 layers over T = 1 or 2 towers as the step takes them: one launch per
 * layer for all towers (slabs [tower][split]), ONE reduce table and slab cursor shared by the layers, one ordered reduction at
 * the end (and one whenever the table is full).  Host arrays: geom [L][9] = N, H, W, Cin, Cout, KH, KW, stride, pad;
 * tensors [L][T][4] = the device pointers x, dy, in_scale, in_shift of each tower (prologue: both vectors for every tower, or none);
 * dw_off [L]: where the layer's dW (OHWI, ACCUMULATED into) starts in `grads`, in floats; bias_off [L][2] or NULL: where the column
 * sums of dy are accumulated (-1 = nowhere; the second is another destination of the same sums, the projection shortcut's bias).
 * Destinations of different layers must not overlap.  workspace: exactly stabnet_conv2d_wgrad_layers_workspace_bytes() are used
 * (0 for a bad geometry).  STABNET_ERR_BAD_ARG, before anything is written: T outside 1..2, a bias on a layer that is not a 1x1
 * stride-1 layer with Cout % 256 == 0 on the stride-1 kernel, a destination outside `grads` or not 16-byte aligned, a workspace
 * that is too small. */
size_t stabnet_conv2d_wgrad_layers_workspace_bytes(int L, int T, const int* geom, const long* bias_off);
int stabnet_conv2d_wgrad_layers(int L, int T, const int* geom, const float* const* tensors, float* grads, size_t grads_floats,
                                const long* dw_off, const long* bias_off, void* workspace, size_t workspace_bytes, void* stream);

/* The dgrad weights of L <= 56 layers by one launch: entry i (host arrays: w_off [L], dims [L][4] = Cout, K, Cin, stride) is
 * params[w_off ...] OHWI [Cout][K][K][Cin]; its re-pack wt[ci][kh][kw][co] = w[co][K-1-kh][K-1-kw][ci] follows entry i - 1's in
 * `wt` (3x3 filters of stride-2 layers keep their tap rows kh in the order 1, 0, 2).  STABNET_ERR_BAD_ARG for L > 56. */
int stabnet_pack_dgrad_weights_table(const float* params, size_t params_floats, float* wt, size_t wt_floats, int L, const long* w_off,
                                     const int* dims, void* stream);

/* stabnet_conv_weight_split_image for L <= 64 matrices by one launch: matrix i (host arrays: dims [L][2] = Cout, K with K % 32 == 0)
 * is w_base[w_off[i] ...] as [Cout][K], its image goes to img_base[img_off[i] ...] (offsets in floats, multiples of 4). */
int stabnet_conv_weight_split_images_table(const float* w_base, size_t w_floats, float* img_base, size_t img_floats, int L,
                                           const long* w_off, const long* img_off, const int* dims, void* stream);

/* stabnet_conv2d_dgrad as the step runs it in operand mode 4: the table re-pack, the image of the re-packed weights where one
 * exists (KH * KW * Cout % 32 == 0; no image otherwise, as in the step) and dgrad on the packed split kernels wherever they take
 * the launch (exact float32 elsewhere).  residual may be dx.  *packed_route (host, optional) = 1 if the launch went to a packed
 * split kernel, 0 if it ran the exact-f32 kernels. */
size_t stabnet_conv2d_dgrad_split_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int stabnet_conv2d_dgrad_split(const float* dy, const float* w_ohwi, float* dx, const float* residual, int N, int H, int W, int Cin,
                               int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t workspace_bytes,
                               int* packed_route, void* stream);

/* ---- training: the regressor tower (get_resnet(is_training=True) and its autodiff) -------------------------
 * The plan must be created with keep_activations = 1.  One workspace per tower (activations are kept between the
 * forward and the backward of the same tower; the siamese step runs two towers, train_bundle_nobm.py:107-108). */
size_t stabnet_net_train_workspace_bytes(const void* net);

/* Forward with batch-statistics BN (tf.nn.moments, biased variance); updates the moving averages stored in `params`
 * (slim UPDATE_OPS tied to the step, s_net_bundle_nobm.py:355-356).  x_tensor [N,H,W,in_ch] -> theta [N,n_theta]. */
int stabnet_tower_fwd_train(const void* net, float* params, const float* x_tensor, float* theta, void* workspace,
                            size_t workspace_bytes, float bn_eps, float bn_decay, void* stream, void* prof);

/* Both siamese towers of a step (train_bundle_nobm.py:107-108: two towers over the same weights) in LOCKSTEP, layer by layer:
 * per layer ONE convolution launch over both towers' batches where the tower's rows are a multiple of the 64-row tile (else the
 * convolution of tower 1, then of tower 2), and ONE batch-statistics reduction launch covering both.  The results are those of
 * tower_fwd_train(x1) then tower_fwd_train(x2) up to float32 summation order (the pair's launch may choose another split-K);
 * the moving averages receive tower 1's update, then tower 2's.  One workspace per tower. */
int stabnet_towers_fwd_train(const void* net, float* params, const float* x1, const float* x2, float* theta1, float* theta2,
                             void* workspace1, void* workspace2, size_t workspace_bytes, float bn_eps, float bn_decay,
                             void* stream, void* prof);

/* Backward from d_theta [N,n_theta]; parameter gradients are ACCUMULATED into grads (layout = trainable prefix of
 * params; zero once per step). */
int stabnet_tower_bwd(const void* net, const float* params, const float* d_theta, float* grads, void* workspace,
                      size_t workspace_bytes, void* stream, void* prof);
/* The same backward in stabnet_net_num_grad_stages() stages (0: FC head + block4, 1: block3, 2: block2, 3: block1 + stem;
 * call them in this order).  When stage k's kernels are done the gradients in [lo, hi) of stabnet_net_grad_bucket(k) are
 * final for this tower -- a data-parallel host hands that bucket to the collective while the earlier layers are still in
 * backward (reverse layer order).  The BN gamma / beta sections (stabnet_net_bn_grad_range) are final after the last stage.
 * THE BUCKET CONTRACT (tests/test_bwd_stages_gpu.py, on snapshots of the buffer after every stage call, for this entry and for
 * stabnet_towers_bwd_stage; tests/test_parallel_cpu.py for the layout):
 *   - a stage writes only its own bucket and the BN range: nothing below, nothing above, nothing outside [0, trainable floats);
 *   - an earlier stage's bucket is never touched again -- what stage k leaves there is what the whole backward leaves there;
 *   - every weight and bias tensor of the bucket receives its gradient in that stage (no reduction is left pending), as an ADD
 *     into whatever the buffer held; four stage calls give the bits of one stabnet_tower_bwd;
 *   - the boundaries between stage buckets, and every conv weight / bias offset, are multiples of 4 floats (16 bytes): the float4
 *     read-modify-writes of the slab reduction and of the FC weight gradient cannot reach into a neighbouring bucket.  The
 *     boundary between bucket 0 and the BN range is written with 4-byte scalar accesses on both sides.
 * The stages must be called in the order 0, 1, 2, 3, once each per backward: stage k reads the d(activation) stage k - 1 left in the
 * workspace.  NOTHING ENFORCES THE ORDER -- a call out of order returns STABNET_OK and a wrong gradient. */
int stabnet_tower_bwd_stage(const void* net, const float* params, const float* d_theta, float* grads, void* workspace,
                            size_t workspace_bytes, int stage, void* stream, void* prof);
/* One backward stage of BOTH towers in lockstep (after stabnet_towers_fwd_train): the bucket of stage k then holds the sum of
 * both towers' gradients.  The dgrad weights are re-packed once, the wgrad slabs of both towers are reduced together.
 * PAIRING (checked, STABNET_ERR_BAD_ARG otherwise): the lockstep forward keeps the FC-head activations of both towers in
 * workspace1, the single-tower forward in its own workspace, so stabnet_towers_bwd_stage(ws1, ws2) must follow
 * stabnet_towers_fwd_train(ws1, ws2) on the same two workspaces, and stabnet_tower_bwd / _bwd_stage(ws) must follow
 * stabnet_tower_fwd_train(ws). */
int stabnet_towers_bwd_stage(const void* net, const float* params, const float* d_theta1, const float* d_theta2, float* grads,
                             void* workspace1, void* workspace2, size_t workspace_bytes, int stage, void* stream, void* prof);
int stabnet_net_num_grad_stages(void);
int stabnet_net_grad_bucket(const void* net, int stage, long* lo, long* hi);
int stabnet_net_bn_grad_range(const void* net, long* lo, long* hi);

/* Float offsets, inside a tower workspace, of the batch BN buffers [G] (scale, shift, mean, invstd) of the last forward. */
int stabnet_net_train_bn_offsets(const void* net, long* scale_off, long* shift_off, long* mean_off, long* invstd_off);

/* Debug view of a training workspace after a forward (tests read the forward's discrete decisions -- ReLU signs, max-pool
 * argmax -- back from it): what = "bn:<channel offset>" (the tensor that BN normalises: float offset, M*C elements),
 * "fcx0".."fcx3" (input of FC layer k of the PAIR, [2N][dims[k]], tower 0's workspace), "argmax" (float offset of the pool's
 * argmax bytes, byte count), "pool". */
int stabnet_net_train_debug_offset(const void* net, const char* what, long* off, long* count);

/* ---- training: the non-convolution layers of the tower, one entry per operator ------------------------------
 * The launchers that stabnet_tower(s)_fwd_train / _bwd* run (slim resnet_v2_50 + FC head under is_training=True and their
 * autodiff: s_net_bundle_nobm.py:252-258, minimised at train_bundle_nobm.py:160), reachable one at a time.  Tensors are
 * [M][C] row-major (M = N*H*W pixels, C % 4 == 0).  groups = 1 | 2: the same operator on both siamese towers in one launch each
 * (train_bundle_nobm.py:107-108); the arguments ending in 1 are read only when groups = 2.  Every sum is taken in a fixed order
 * (no atomics): the same call gives the same bits, and groups = 2 gives the bits of two groups = 1 calls in order.
 * `partial`: stabnet_col_reduce_workspace_floats(M, C, groups) floats (0 = bad arguments). */
size_t stabnet_col_reduce_workspace_floats(long M, int C, int groups);

/* slim batch_norm(is_training=True) statistics (resnet_v2.resnet_arg_scope, s_net_bundle_nobm.py:252): tf.nn.moments over the M
 * rows -> stats [4][C] per group = {scale = gamma * invstd, shift = beta - mean * scale, mean, invstd = 1 / sqrt(var + eps)} with
 * the BIASED variance, and the moving averages mov -= (mov - value) * (1 - decay) (UPDATE_OPS, s_net_bundle_nobm.py:355-356;
 * group 0's update, then group 1's; both NULL = left alone).
 * Conditioning: the variance is formed as E[x^2] - mean^2 in one pass, not in the two passes of tf.nn.moments, which amplifies
 * the rounding of the two sums by 1 + r^2, r = |mean| / std of the channel.  The sums are therefore taken in float64 (float32
 * products are exact there): the variance error stays inside (1 + r^2) * 2^-23 -- asserted per channel for r = 0 .. 100 at every
 * layer size of the 8 x 288 x 512 step -- and is in fact the rounding of the float32 result, 2^-24, up to r ~ 10^4.
 * partial must be 8-byte aligned. */
int stabnet_bn_stats_train(int groups, const float* x0, const float* x1, long M, int C, const float* gamma, const float* beta,
                           float eps, float decay, float* stats0, float* stats1, float* mov_mean, float* mov_var, float* partial,
                           void* stream);

/* Autodiff of relu(batch_norm(x)) with batch statistics (the preact / conv BN + ReLU sites of resnet_v2 `bottleneck`):
 * dz = g * (fma(x, scale, shift) > 0), xhat = (x - mean) * invstd,
 * d_x = gamma * invstd * (dz - mean_M(dz) - xhat * mean_M(dz * xhat)) (+ addend), d_gamma += sum dz * xhat, d_beta += sum dz
 * (both ACCUMULATED into, group 0 then group 1).  stats: what stabnet_bn_stats_train wrote.  d_x may alias g.
 * addend (optional, NULL): the gradient arriving over the identity shortcut; add_stride = 1: [M][C]; add_stride = s > 1 (slim
 * `subsample`): [N][ceil(H/s)][ceil(W/s)][C], added at the pixels with y % s == 0 and x % s == 0 (H, W are read only then,
 * M = N*H*W).  coef: [3][C] floats of scratch per group. */
int stabnet_bn_relu_bwd(int groups, const float* x0, const float* x1, const float* g0, const float* g1, const float* stats0,
                        const float* stats1, const float* gamma, long M, int C, const float* addend0, const float* addend1,
                        int add_stride, int H, int W, float* d_gamma, float* d_beta, float* d_x0, float* d_x1, float* partial,
                        float* coef0, float* coef1, void* stream);

/* d_bias [C] += column sums of g (group 0 then group 1) -- autodiff of slim conv2d's bias add; d_bias2 (optional, NULL) receives
 * the same increment: the conv3 and projection-shortcut biases of a unit add into the same tensor. */
int stabnet_bias_grad(int groups, const float* g0, const float* g1, long M, int C, float* d_bias, float* d_bias2, float* partial,
                      void* stream);

/* slim max_pool2d [3,3] stride 2 of resnet_v2 ('pool1'), training form: y [N,Ho,Wo,C] and argmax bytes [N,Ho,Wo,C] = dy*k + dx of
 * the FIRST maximum in scan order (rows, then columns) over the in-image taps of the window at (oy*stride - pt, ox*stride - pl).
 * Backward (gather, no atomics): dx [N,H,W,C] = sum of the dy of every window whose argmax points at the pixel (written, not
 * accumulated).  k*k <= 255. */
int stabnet_max_pool_train_fwd(const float* x, float* y, unsigned char* argmax, int N, int H, int W, int C, int Ho, int Wo, int k,
                               int stride, int pt, int pl, void* stream);
int stabnet_max_pool_bwd(const unsigned char* argmax, const float* dy, float* dx, int N, int H, int W, int C, int Ho, int Wo, int k,
                         int stride, int pt, int pl, void* stream);

/* Autodiff of tf.reduce_mean(resnet, [1, 2]) (s_net_bundle_nobm.py:254): da [N,HW,C] = dg [N,C] / HW (one float32 division). */
int stabnet_gap_bwd(const float* dg, int N, int HW, int C, float* da, void* stream);

/* Autodiff of slim.fully_connected (s_net_bundle_nobm.py:256-258 with ReLU, the output layer without): x [M,K], w [Nout][K],
 * y [M,Nout] = the layer's output (relu = 1; NULL when relu = 0), dy [M,Nout].  dyr = dy * (y > 0) when relu;
 * dW [Nout][K] += dyr^T x, db [Nout] += column sums of dyr (both ACCUMULATED into), dx [M,K] = dyr w (written; NULL = not
 * wanted).  K % 4 == 0.  scratch: stabnet_fc_bwd_scratch_floats(M, K, Nout) floats, read and written only when dx is given;
 * a smaller one is refused (STABNET_ERR_BAD_ARG) before anything is launched. */
size_t stabnet_fc_bwd_scratch_floats(int M, int K, int Nout);
int stabnet_fc_bwd(const float* x, const float* w, const float* y, const float* dy, int M, int K, int Nout, int relu, float* dW,
                   float* db, float* dx, float* scratch, size_t scratch_floats, void* stream);

/* slim L2 regularisers (REGULARIZATION_LOSSES, s_net_bundle_nobm.py:324-325; resnet.py:35-37): *loss_out +=
 * sum_seg coef*0.5*sum w^2 (NULL to skip), grads[seg] += gscale*coef*w (NULL to skip).  seg_* are DEVICE arrays.
 * workspace: 64*nseg floats (block partials of the value; may be NULL when loss_out is). */
int stabnet_weight_decay(const float* params, float* grads, const long* seg_off, const long* seg_len,
                         const float* seg_coef, int nseg, float gscale, float* loss_out, float* workspace, void* stream);

/* tf.train.AdamOptimizer step (train_bundle_nobm.py:155-160): g = (grads + grads2) * gscale (grads2 may be NULL). */
int stabnet_adam_step(float* params, const float* grads, const float* grads2, float* m, float* v, long n, float lr,
                      float beta1, float beta2, float eps, int step, float gscale, void* stream);

/* ---- next to the path: colour-frame remap with smoothed maps --------------------------
 * warpRevBundle2(img, x_map, y_map) (deploy_bundle.py:136-146,303): cv2.resize of both maps down by `rate` and back
 * up (INTER_LINEAR), (m+1)/2*size, cv2.remap(img, ., ., INTER_LINEAR) of the uint8 BGR frame.  img, out uint8
 * [N,H,W,C]; x_map, y_map [N,H,W]; workspace 2*N*(H/rate)*(W/rate) floats; px_out, py_out optional [N,H,W]. */
int stabnet_warp_rev_bundle2(const unsigned char* img, const float* x_map, const float* y_map, int N, int H, int W, int C,
                             int rate, unsigned char* out, float* workspace, float* px_out, float* py_out, void* stream);

/* The same remap at SOURCE resolution: the frame as read, of any size, warped by the network-size maps (nothing in the reference:
 * it resizes the colour frame down to the network's size first, deploy_bundle.py:303).  src uint8 [N,SH,SW,C], C = 3 BGR or 1 grey,
 * rows row_stride_bytes apart (>= SW*C), frames SH*row_stride_bytes apart, any base alignment; nothing outside
 * [src, src + (SH-1)*stride + SW*C) of a frame is read.  x_map, y_map [N,H,W] normalised, h = H/rate, w = W/rate:
 *   small = cv2.resize(map, (w, h));  big = cv2.resize(small, (SW, SH));  ux = (big_x + 1)/2*W, uy = (big_y + 1)/2*H;
 *   px = ux*sx + cx, py = uy*sy + cy  (float32 multiply, then add; sx = float32(SW/W), cx = float32(0.5*SW/W - 0.5), likewise y, from double:
 *   cv2's half-pixel convention -- the normalised coordinate counts pixel indices, so cx is what keeps an identity mesh in place);
 *   out = cv2.remap(src, px, py, INTER_LINEAR), BORDER_CONSTANT 0, the fixed-point path of stabnet_warp_rev_bundle2.
 * With SH, SW == H, W the results are stabnet_warp_rev_bundle2's bit for bit.  out uint8 [N,SH,SW,C] dense.  black_count (optional,
 * int32 [N,SH,SW], what stabnet_crop_search reads): += 1 where the coordinate rounded to 1/32 px lies outside the frame
 * (qx < 0 || qx > 32*(SW-1) || qy < 0 || qy > 32*(SH-1); NaN maps too) -- a read-modify-write of black pixels only, by the pixel's
 * own thread.  px_out/py_out optional [N,SH,SW], both or neither.  workspace 2*N*h*w floats.  SH, SW in 1..32767 (the remap's
 * 16-bit pixel index).  Two launches; nothing allocates, synchronises or copies from the host.  STABNET_REMAP_VEC4=0 selects the
 * one-pixel-per-thread kernel, as in stabnet_warp_rev_bundle2. */
int stabnet_warp_rev_bundle2_src(const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes,
                                 const float* x_map, const float* y_map, int H, int W, int rate,
                                 unsigned char* out, int* black_count, float* workspace,
                                 float* px_out, float* py_out, void* stream, void* prof);

/* The same remap through a WINDOW of the stabilised frame (crop and zoom in the one gather; remap_win_kernel / remap_win4_kernel).
 * The contract is stabnet_warp_rev_bundle2_src's, except that the output has its own size OH x OW (1..32767) and output pixel (i, j)
 * is the stabilised frame, at SH x SW, sampled at a fractional position inside window = {y0, x0, wh, ww}: four doubles in HOST memory,
 * read during the call, in pixel-edge units of the stabilised frame -- the window covers [x0, x0 + ww) x [y0, y0 + wh), the whole
 * frame is {0, 0, SH, SW}.  With w = W / rate, h = H / rate:
 *   ex = x0 + ((double)j + 0.5) * (ww / OW)           double: the quotient, the product, the sum
 *   f  = (float)(ex * ((double)w / SW) - 0.5)         then cv2.resize's taps: floor, border clamps with the weight zeroed
 * and likewise ey from y0, wh, OH, h, SH; from there on every step is _src's.  Hence bit for bit: the whole-frame window at
 * OH, OW == SH, SW gives _src's frame, coordinates and counts, and an integer window with ww == OW, wh == OH gives the slice
 * [y0 : y0 + OH, x0 : x0 + OW] of them.  out uint8 [N,OH,OW,C] dense; black_count, px_out, py_out [N,OH,OW], at the OUTPUT pixel
 * under _src's rule.  The four-pixel kernel needs C == 3, OW % 4 == 0 and a 4-byte aligned out (16-byte px_out / py_out); the
 * source may have any width, stride and alignment.  Refused: everything _src refuses, a null window, a non-finite entry,
 * wh <= 0 or ww <= 0, a window that leaves [0, SH] x [0, SW] by more than 1e-6 px. */
int stabnet_warp_rev_bundle2_win(const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes,
                                 const float* x_map, const float* y_map, int H, int W, int rate,
                                 const double* window, int OH, int OW,
                                 unsigned char* out, int* black_count, float* workspace,
                                 float* px_out, float* py_out, void* stream, void* prof);

/* stabnet_warp_rev_bundle2_win with the window in DEVICE memory (remap_win_dev_kernel / remap_win4_dev_kernel: the bodies of the _win
 * kernels): window double [N,4], {y0, x0, wh, ww} per stream, loaded by the kernels when they RUN -- so an earlier launch on the stream
 * (stabnet_fill_window_update) may write it, and a captured graph replays with whatever it holds then.  The kernels form
 * xstep = ww / OW and ystep = wh / OH in double (IEEE division: the host's bits), hence frame, coordinates and counts are _win's bit
 * for bit for the same window.  The window's VALUES cannot be refused by the host: a stream whose window has a non-finite entry,
 * wh <= 0 or ww <= 0, or leaves [0, SH] x [0, SW] by more than 1e-6 px, is read through the whole frame {0, 0, SH, SW}; no tap is
 * ever derived from a NaN.  Everything else -- the other refusals, the choice between the two kernels, STABNET_REMAP_VEC4,
 * black_count / px_out / py_out -- is _win's. */
int stabnet_warp_rev_bundle2_win_dev(const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes,
                                     const float* x_map, const float* y_map, int H, int W, int rate,
                                     const double* window, int OH, int OW,
                                     unsigned char* out, int* black_count, float* workspace,
                                     float* px_out, float* py_out, void* stream, void* prof);

/* stabnet_warp_rev_bundle2_win of a planar YUV 4:2:0 frame as a Y4M stream carries it (remap_i420_kernel): no colour conversion, every
 * plane warped as the single-channel image it is, all planes of all frames in one gather launch after the shrink.
 * src: N frames frame_stride_bytes apart; each the Y plane [SH,SW] and, with planes == 3, U [SH/2,SW/2] and V [SH/2,SW/2] behind it,
 * all dense (planes == 1: Y only).  Any base alignment; nothing outside a frame's own SH*SW*3/2 (SH*SW) bytes is read.  out: the same
 * layout at OH x OW, dense.  window: {y0, x0, wh, ww} in HOST memory, pixel-edge units of the stabilised LUMA frame, as _win takes it,
 * or NULL: the whole frame, and then OH, OW must equal SH, SW.
 * Each plane is what _win gives that plane as a C == 1 image of its own size: Y at (SH,SW) -> (OH,OW) through `window`, a chroma plane
 * at (SH/2,SW/2) -> (OH/2,OW/2) through {y0/2, x0/2, wh/2, ww/2}, with the plane's own constants sx = float32((SW/2)/W),
 * cx = float32(0.5*(SW/2)/W - 0.5) (centred chroma siting: the luma coordinate of the chroma sample, halved).  One difference: a tap
 * outside the plane reads a border value instead of 0 (cv2.remap's borderValue): border_y (0..255) for Y, 128 for U and V.  The 1/32-px
 * rounding, the 15-bit weights with the (0, 0) repair and (sum + 16384) >> 15 are unchanged.  black_count (optional, int32 [N,OH,OW]):
 * += 1 at the LUMA output pixel under _src's rule.  workspace: 2*N*(H/rate)*(W/rate) floats.
 * One workgroup per output row segment of one plane; a plane whose output width is a multiple of 4 and whose output rows are 4-byte
 * aligned takes four pixels per thread and one dword store, any other one pixel per thread with byte traffic (STABNET_REMAP_VEC4=0:
 * every plane); the bits are the same.  Nothing allocates, synchronises or copies: the call can be captured in a hipGraph.
 * Refused before any launch: null src, out, maps or workspace; planes not 1 or 3; odd SH, SW, OH or OW with planes == 3; sizes outside
 * 1..32767; frame_stride_bytes below the frame's size; border_y outside 0..255; rate < 1 or H/rate or W/rate == 0; a null window with
 * OH, OW != SH, SW; a window _win would refuse. */
int stabnet_warp_rev_bundle2_i420(const unsigned char* src, int N, int SH, int SW, int planes, size_t frame_stride_bytes,
                                  const float* x_map, const float* y_map, int H, int W, int rate,
                                  const double* window, int OH, int OW, int border_y,
                                  unsigned char* out, int* black_count, float* workspace, void* stream, void* prof);

/* The remaps above with cv2.remap's INTER_CUBIC in place of INTER_LINEAR (remap_cubic_kernel<PX, KIND>; tests/remap_cubic_model.py).
 * Coordinates, their quantisation to 1/32 px (qx, qy), coverage, px_out/py_out, the refusals and the choice between the one- and the
 * four-pixel kernel are the bilinear entries'; only the taps and the blend differ.  With ix = sat16(qx >> 5), fx = qx & 31 (same in y):
 *   taps   rows iy - 1 .. iy + 2, columns ix - 1 .. ix + 2; a tap outside the frame reads 0 (BORDER_CONSTANT)
 *   1-D    c[0..3] = interpolateCubic(f / 32), A = -0.75, float32, left to right, not contracted
 *   w      [k1][k2] = saturate_cast<short>(rint(float32(cy[k1] * cx[k2]) * 32768)); an entry whose 16 taps do not sum to 32768 is
 *          repaired as initInterTab2D does: over taps k1, k2 in {2, 3} in row order the minimum (strict <) or else the maximum
 *          (strict >), both starting at [2][2]; diff = sum - 32768 < 0 is taken from the maximum, otherwise from the minimum
 *   out    clamp((sum(v * w) + 16384) >> 15, 0, 255)      int32 accumulator: sum |w| <= 61952
 * The kernels read the 1024 x 16 int16 table as a constant of the code object, compiled from this rule (no upload, no state per
 * device).  Not separable: a two-pass form rounds differently.  window_kind 0: the whole frame at its own size (window not read, OH, OW must equal SH, SW; with SH, SW == H, W this is
 * the network-size remap), 1: window = {y0, x0, wh, ww} in HOST memory as _win takes it, 2: window double [N,4] in DEVICE memory as
 * _win_dev takes it (values _win would refuse give the whole frame).  Two launches. */
int stabnet_warp_rev_bundle2_cubic(const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes,
                                   const float* x_map, const float* y_map, int H, int W, int rate,
                                   int window_kind, const double* window, int OH, int OW,
                                   unsigned char* out, int* black_count, float* workspace,
                                   float* px_out, float* py_out, void* stream, void* prof);

/* stabnet_warp_rev_bundle2_i420 with the bicubic taps on every plane (remap_i420_kernel<true>): a tap outside a plane reads border_y
 * (Y) or 128 (U, V); the weights sum to 32768, so that is cv2.remap's borderValue form.  Everything else as _i420. */
int stabnet_warp_rev_bundle2_i420_cubic(const unsigned char* src, int N, int SH, int SW, int planes, size_t frame_stride_bytes,
                                        const float* x_map, const float* y_map, int H, int W, int rate,
                                        const double* window, int OH, int OW, int border_y,
                                        unsigned char* out, int* black_count, float* workspace, void* stream, void* prof);

/* The 1024 x 16 weights of the bicubic remap, entry fy * 32 + fx, tap k1 * 4 + k2, int16.  _table: built on the host by the function
 * the kernels' table is compiled from, at run time (no GPU needed).  _weights_dev: out_dev in device memory, written by one launch,
 * every phase exactly as the remap kernels obtain it (read from their table). */
int stabnet_remap_cubic_table(short* out);
int stabnet_remap_cubic_weights_dev(short* out_dev, void* stream);

/* Adaptive borderless output: per stream, the largest centred window of the stabilised frame that is provably free of uncovered
 * pixels, rate-limited on the way back out (fill_window_kernel).  x_map, y_map [N,H,W] as the remap receives them; h = H / rate,
 * w = W / rate.  Node (a, b) of the h x w small maps is BAD when its own coordinate (the remap's arithmetic with all the weight on the
 * node) rounded to 1/32 px has qx < margin_q, qx > 32*(SW-1) - margin_q, or the same in y (a NaN entry: -2e9, bad).  Every output
 * coordinate is a convex combination of its four nodes, so a window that reads no bad node shows no uncovered pixel:
 *   key(a, b) = max((|2b+1-w| - 2) * h, (|2a+1-h| - 2) * w)      key = min over the bad nodes, h*w when there is none   (int32)
 *   r_safe = key >= h*w ? 1.0 : (double)key / (double)(h*w)      (may be <= 0)
 *   r = fmin(r_safe, state[n] + up);  r = fmax(r, r_min);  r = fmin(r, 1.0);  state[n] = r
 *   wh = SH*r;  ww = SW*r;  window[n] = {(SH - wh)/2, (SW - ww)/2, wh, ww};  stats[n] = {key, number of bad nodes}
 * state double [N] (set to 1.0 at the start of a clip), window double [N,4], stats int32 [N,2], workspace 2*N*h*w floats: device
 * memory.  Two launches (the shrink; one workgroup per stream, shuffles and LDS, no atomics): deterministic, nothing allocates,
 * synchronises or copies.  Refused before any launch: null pointers, the sizes _src refuses, more than 2^30 nodes, r_min outside
 * (0, 1], up negative or not finite, margin_q outside 0..16*min(SH, SW). */
int stabnet_fill_window_update(const float* x_map, const float* y_map, int N, int H, int W, int rate, int SH, int SW,
                               double r_min, double up, int margin_q, double* state, double* window, int* stats,
                               float* workspace, void* stream);

/* cvt_train2img (deploy_bundle.py:75): the network's grey output back to 8 bits, out[i] = uint8((x[i] + 0.5) * 255) clipped to
 * [0, 255].  x float [n], out uint8 [n].  The 16-byte path needs both pointers 16-byte aligned (any alignment is accepted). */
int stabnet_cvt_train2img(const float* x, unsigned char* out, long n, void* stream);

/* ---- next to the path: max-inscribed-rectangle crop --------------------------------
 * deploy_bundle.py:291: all_black += round(black) per frame;  :344-366: once per video, the largest black-free rectangle
 * whose top-left corner lies on the `step` (10) grid of the top-left quadrant, first-found-wins on ties. */
int stabnet_black_accumulate(const float* black, int* all_black, long n, void* stream);
size_t stabnet_crop_search_workspace_bytes(int H, int W, int step);
int stabnet_crop_search(const int* all_black, int H, int W, int step, int* ans5, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---- next to the path: training sample assembly -------------------------------------
 * read_and_decode's tensor part (get_data_mini_after.py:229-253) for N pairs at once: warp_img (:14-31: bilinear up-scale
 * by 1/random_crop_rate, crop, flip, tf.image contrast + brightness, clip) on the 2*(before_ch+1) stable and 2 unstable
 * channels, add_mask (:93-147: random-homography black masks, masked pixels = -1), warp_flow (:33-51), warp_point
 * (:53-70).  The random draws are INPUTS (device arrays): para [N][3] = crop row, crop column, flip; jitter [N][2] =
 * contrast factor, brightness delta; Hs [N][2][before_ch][9] mask homographies (tower, channel).
 * stable [N,H,W,2*(before_ch+1)] (label, history x before_ch, per tower), unstable [N,H,W,2], flow [N,H,W,2] (or NULL),
 * matches [N,max_matches,4] + n [N] valid counts (or NULL).  Outputs NHWC: x1,x2 [N,H,W,2*before_ch+1] (masks, masked
 * history, current), y1,y2 [N,H,W,1], flow_out, fm [N,max_matches,4], mk [N,max_matches] (0/1 floats).
 * random_crop_rate is a double, in (0, 1]: the resized size is (int)(H / rate), (int)(W / rate) in float64, the number Python's
 * int(height / random_crop_rate) gives and the host draws its crop offsets for (a rate rounded to float32 first gives another
 * size: 288 / 0.8 = 360, 288 / 0.8f = 359).  para lives on the device where the entry cannot inspect it, so the kernels clamp
 * the crop row to [0, (int)(H / rate) - H] and the crop column to [0, (int)(W / rate) - W] (a legal draw is unchanged; an illegal
 * one gives the result of the nearest legal one instead of a read outside the inputs), and flip means para[n][2] != 0.
 * stable and unstable must be 8-byte aligned; every argument is checked before the first launch. */
size_t stabnet_augment_workspace_bytes(int N, int H, int W, int before_ch);
int stabnet_augment_pairs(const float* stable, const float* unstable, const float* flow_in, const float* matches1,
                          const int* n1, const float* matches2, const int* n2, const int* para, const float* jitter,
                          const float* Hs, int N, int H, int W, int before_ch, int max_matches, double random_crop_rate,
                          float* x1, float* y1, float* x2, float* y2, float* flow_out, float* fm1, float* mk1, float* fm2,
                          float* mk2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- after the path: Motion-JPEG encoding of the stabilised frame (deploy_bundle.py:197-198,305: VideoWriter 'MJPG') ----
 * Baseline JFIF (SOF0, 8-bit, the four Annex K Huffman tables, restart intervals) encoded where the frame lies.
 * img uint8 [N,H,W,C]: C = 3 BGR (what stabnet_warp_rev_bundle2 writes) or C = 1 grey (stabnet_cvt_train2img); any H, W in
 * 1..65535, partial MCUs replicate the last row / column.  subsampling 420 (MCU 16x16, chroma = mean of 2x2) or 444 (MCU 8x8);
 * ignored for C = 1.  Colour: JFIF full-range BT.601 in float32, not rounded to 8 bits before the orthonormal float32 DCT;
 * q = rint(coef / Q), AC clamped to +-1023 and DC to +-1024.  restart_mcus (1..65535) = DRI: every interval starts byte-aligned
 * with DC predictors 0, ends padded with 1-bits and is followed by RSTm (m mod 8) -- the intervals are coded in parallel.
 * Every buffer is sized for the worst case of a block (416 bytes with every byte stuffed), so there is no overflow to report:
 * out_bytes[n] <= stabnet_mjpeg_max_bytes always.  Nothing allocates, synchronises or copies from the host inside encode. */
int stabnet_jpeg_quant_tables(int quality, unsigned short* luma64, unsigned short* chroma64);   /* host; IJG scaling of Annex K, quality 1..100, natural order */
/* host; SOI .. SOS.  Returns the number of bytes (host_out NULL: only the count), -1 on bad arguments or a cap too small. */
int stabnet_mjpeg_header(int H, int W, int C, int subsampling, int restart_mcus, const unsigned short* luma64,
                         const unsigned short* chroma64, unsigned char* host_out, int cap);
size_t stabnet_mjpeg_max_bytes(int H, int W, int C, int subsampling, int restart_mcus);        /* per frame, header included; 0 = bad arguments */
size_t stabnet_mjpeg_workspace_bytes(int N, int H, int W, int C, int subsampling, int restart_mcus);
/* luma64_dev, chroma64_dev (NULL allowed when C = 1): tables in natural order ON THE DEVICE; header_dev: the header of the same
 * arguments ON THE DEVICE.  out + n * out_stride receives stream n (out_stride >= stabnet_mjpeg_max_bytes), out_bytes[n] its
 * length (device int32).  workspace: 16-byte aligned. */
int stabnet_mjpeg_encode(const unsigned char* img, int N, int H, int W, int C, int subsampling, int restart_mcus,
                         const unsigned short* luma64_dev, const unsigned short* chroma64_dev, const unsigned char* header_dev,
                         int header_bytes, unsigned char* out, size_t out_stride, int* out_bytes, void* workspace,
                         size_t workspace_bytes, void* stream, void* prof);
/* The same streams from a PLANAR frame: src holds N frames frame_stride_bytes apart (>= the frame's size), each Y [H,W] and, for
 * planes = 3, U [H/2,W/2] and V [H/2,W/2] behind it, all dense -- the layout stabnet_warp_rev_bundle2_i420 writes and
 * stabnet_mjpeg_decode_i420 fills.  The samples are taken as the JFIF components they are (full range, chroma centred): the load
 * stage of mjpeg_transform_planar_kernel is the level shift alone, no colour arithmetic and no 2x2 mean; partial MCUs replicate the
 * edge sample of each plane.  Header, tables, stabnet_mjpeg_max_bytes and stabnet_mjpeg_workspace_bytes are those of C = planes,
 * subsampling 420, and every other argument is stabnet_mjpeg_encode's.  planes = 3 needs even H and W; any base pointer and stride
 * are accepted (aligned dwords are read where the address allows).  Refused with STABNET_ERR_BAD_ARG before any launch: planes not 1 | 3,
 * an odd side with planes = 3, a stride below the frame's size, and what stabnet_mjpeg_encode refuses. */
int stabnet_mjpeg_encode_i420(const unsigned char* src, int N, int H, int W, int planes, size_t frame_stride_bytes, int restart_mcus,
                              const unsigned short* luma64_dev, const unsigned short* chroma64_dev, const unsigned char* header_dev,
                              int header_bytes, unsigned char* out, size_t out_stride, int* out_bytes, void* workspace,
                              size_t workspace_bytes, void* stream, void* prof);

/* ---- in front of the ingest: Motion-JPEG decoding of the frame as read (the reference reads its clips with cv2.VideoCapture) ----
 * Baseline JPEG (SOF0, 8-bit samples, 8-bit DQT, Huffman tables of the stream's own DHT or Annex K when it has none; grey 1x1,
 * 4:4:4, 4:2:0; one interleaved scan; any restart interval) decoded on the device, bit for bit what libjpeg-turbo's default decoder
 * (JDCT_ISLOW, fancy upsampling: what Pillow and OpenCV run) gives: T.81 entropy decoding, dequantisation, jidctint's 13-bit integer
 * IDCT, + 128, clamp; h2v2 fancy upsampling with the neighbours clamped at the true chroma size ceil(H/2) x ceil(W/2); jdcolor's
 * 16-bit fixed-point YCbCr -> RGB, stored B, G, R.  RANGE: libjpeg looks the IDCT's result up in a table that wraps (& 1023) for
 * values no real encoder produces; here it is a plain clamp to [0, 255].
 * Host side (plain C++, no GPU): stabnet_mjpeg_parse reads SOI, DQT, SOF0, DHT, DRI, SOS and scans for the restart markers.  It
 * returns 0, STABNET_MJPEG_UNSUPPORTED = 1 (progressive / any SOF but 0, arithmetic coding, 12-bit samples, 16-bit DQT, 4:2:2 or any
 * other sampling, several scans, Huffman table ids above 1, Adobe / RGB colour, a restart marker count that disagrees with DRI) or -1
 * (not a JPEG stream, truncated, no EOI; bad arguments).  info16: H, W, C, subsampling (420 | 444; 0 grey), DRI (0: none), intervals,
 * MCUs, offset of the scan data, offset of EOI, blob bytes, 1 if the stream has a DHT, blocks.  blob (may be NULL: only info16;
 * 4-byte aligned, blob_cap >= info16[9], at most stabnet_mjpeg_decode_blob_bytes): what the kernels read -- geometry, table
 * selectors, quantiser tables in natural order, four Huffman tables as 9-bit lookup + maxcode / valptr / huffval, and the offset of
 * every restart interval.  stabnet_mjpeg_entropy_host decodes the coefficients (int16 [mcu][block of the MCU][64], natural order, not
 * dequantised; coef_count >= 64 * info16[11]) on the CPU with the routine the entropy kernel runs -- for streams without DRI, which
 * are one interval; -1 when the scan does not decode.
 * Device side: slot n of `in` (in + n * in_stride; both 16-byte aligned) holds the blob at offset 0 and, at offset
 * stabnet_mjpeg_decode_blob_bytes, the whole stream (coef_uploaded = 0) or the coefficients of stabnet_mjpeg_entropy_host
 * (coef_uploaded = 1: no entropy launch).  out uint8 [N,H,W,C] with rows row_stride bytes and frames frame_stride bytes apart (what
 * stabnet_ingest_* reads); status int32 [N] on the device: 0, or the OR of 1 (an interval's bytes ran out), 2 (no such Huffman
 * code), 4 (a run past coefficient 63), 8 (the blob does not fit H, W, C, subsampling or in_stride).  Every byte read is bounded by
 * its interval, every coefficient index by 63, every block by its interval's count: whatever the bytes are, nothing is read or
 * written out of bounds; a lane that meets a violation sets the status and stops.  stages: 3 = the frame; 2 = stop after the IDCT
 * (planes in the workspace), 1 = after the entropy decoding (coefficients in the workspace) -- for tests.  One memset node (status)
 * and three launches (two with coef_uploaded); nothing allocates, synchronises or copies from the host inside decode. */
size_t stabnet_mjpeg_decode_blob_bytes(int H, int W, int C, int subsampling);                    /* host; 0 = bad arguments */
int stabnet_mjpeg_parse(const unsigned char* jpeg, size_t nbytes, int* info16, unsigned char* blob, size_t blob_cap);       /* host */
int stabnet_mjpeg_entropy_host(const unsigned char* jpeg, size_t nbytes, const unsigned char* blob, size_t blob_bytes, short* coef,
                               size_t coef_count);                                                                          /* host */
size_t stabnet_mjpeg_decode_workspace_bytes(int N, int H, int W, int C, int subsampling);
/* host; layout10: per-frame workspace bytes, offset of the coefficients, blocks, offsets of the Y, Cb, Cr planes, Y rows, Y row
 * bytes, chroma rows, chroma row bytes (planes at MCU-padded size). */
int stabnet_mjpeg_decode_layout(int H, int W, int C, int subsampling, size_t* layout10);
int stabnet_mjpeg_decode(const unsigned char* in, size_t in_stride, int N, int H, int W, int C, int subsampling, int coef_uploaded,
                         unsigned char* out, size_t row_stride, size_t frame_stride, int* status, void* workspace, size_t workspace_bytes,
                         int stages, void* stream);
/* The second entropy back end: streams WITHOUT restart markers (one interval: what OpenCV, ffmpeg and cameras write) decoded on the
 * device from the uploaded bytes, in parallel, by self-synchronising Huffman decoding (csrc/jpeg_sync.h).  The interval's bytes are
 * cut into chunks of chunk_bytes; one lane per chunk decodes from a guessed parse state (bit position, block of the MCU, zig-zag
 * index), lanes hand their exit states to the chunk behind them for at most `rounds` rounds inside a workgroup and once across
 * workgroups, and an entry state is accepted only if it is the exit of the accepted walk in front of it -- so what is accepted is the
 * sequential decode; one lane per frame walks again whatever the rounds left unaccepted.  Per-chunk block counts and DC sums are
 * scanned and a second walk writes the coefficients: exactly those of stabnet_mjpeg_entropy_host, hence the pixels of
 * stabnet_mjpeg_decode.  stabnet_mjpeg_decode_sync takes the arguments of stabnet_mjpeg_decode without coef_uploaded (slot = blob |
 * stream), plus chunk_bytes (0 = default; a multiple of 4 in 8..4096), rounds (-1 = default, 0 = repair only, at most 1024) and
 * stats (NULL, or int32 [N][2] on the device: chunks, chunks accepted as the rounds left them -- the repair walked the others; 0 0 for a
 * refused blob).  A frame whose
 * blob has more than one interval gets status 8.  Blocks the stream codes beyond the frame's count are dropped, fewer give status 1.
 * The workspace is stabnet_mjpeg_decode's followed by the chunk states: stabnet_mjpeg_decode_sync_workspace_bytes (0 = bad
 * arguments).  One memset node and four launches (three with rounds = 0) in front of the IDCT and colour launches; the count is
 * fixed at enqueue time and nothing allocates, synchronises or copies from the host.  stages -1, -2, -3 (for measurements: the
 * coefficients are not complete) stop after the guess launch, after the hand-over, after the repair and scan.
 * stabnet_mjpeg_entropy_sync_host: the same phases with the lanes in a loop on the CPU, for tests (chunk_bytes >= 1; stats NULL or
 * int [2]); arguments and result as stabnet_mjpeg_entropy_host, -1 also for a blob of several intervals. */
size_t stabnet_mjpeg_decode_sync_workspace_bytes(int N, int H, int W, int C, int subsampling, size_t in_stride, int chunk_bytes);
int stabnet_mjpeg_decode_sync(const unsigned char* in, size_t in_stride, int N, int H, int W, int C, int subsampling, unsigned char* out,
                              size_t row_stride, size_t frame_stride, int* status, void* workspace, size_t workspace_bytes, int stages,
                              int chunk_bytes, int rounds, int* stats, void* stream);
int stabnet_mjpeg_entropy_sync_host(const unsigned char* jpeg, size_t nbytes, const unsigned char* blob, size_t blob_bytes, short* coef,
                                    size_t coef_count, int chunk_bytes, int rounds, int* stats);                            /* host */
/* The decoder's planes as they are, for the planar warp and the planar encoder: stabnet_mjpeg_decode / _sync without the colour stage.
 * The arguments of the twin without row_stride and stages, plus prof (NULL, or a profiler: only the new launch is recorded).  out
 * receives N frames frame_stride_bytes apart, each Y [H,W] followed, for C = 3, by U (Cb) [H/2,W/2] and V (Cr) [H/2,W/2], all dense:
 * what stabnet_warp_rev_bundle2_i420 reads.  The entropy and IDCT launches are the twin's; mjpegd_planes_kernel then crops the
 * MCU-padded planes to the frame (no arithmetic: Y is libjpeg-turbo's Y exactly, Cb / Cr are the samples its upsampler starts from).
 * Any out pointer and any stride >= the frame's size are accepted; nothing outside a frame's own H * W * 3 / 2 (grey: H * W) bytes
 * is written.  Taken: grey streams of any size, 4:2:0 streams with even H and W.  Refused with STABNET_ERR_BAD_ARG before any launch:
 * 4:2:0 with an odd side, 4:4:4 (both keep the BGR entries), a stride below the frame's size, null pointers, and what the twin
 * refuses.  The workspace is the twin's.  The status words are zeroed by a launch of their own instead of the twins' memset node. */
int stabnet_mjpeg_decode_i420(const unsigned char* in, size_t in_stride, int N, int H, int W, int C, int subsampling, int coef_uploaded,
                              unsigned char* out, size_t frame_stride_bytes, int* status, void* workspace, size_t workspace_bytes, void* stream,
                              void* prof);
int stabnet_mjpeg_decode_sync_i420(const unsigned char* in, size_t in_stride, int N, int H, int W, int C, int subsampling, unsigned char* out,
                                   size_t frame_stride_bytes, int* status, void* workspace, size_t workspace_bytes, int chunk_bytes, int rounds,
                                   int* stats, void* stream, void* prof);

/* ---- in front of the path: frame ingest (config.py:6-21 cvt_img2train; deploy_bundle.py:215,303 cv2.resize) ----
 * A uint8 frame as read from the video, of any size, to the network's grey input and the network-size colour frame.
 * img uint8 [N,sh,sw,C], C = 3 BGR or C = 1 grey, rows row_stride_bytes apart (>= sw*C), frames sh*row_stride_bytes apart.  Every
 * base pointer and row stride is accepted: aligned dwords are read where the address allows, bytes otherwise, and nothing
 * outside the rows themselves.
 * Grey: g = (b*wb + g*wg + r*wr + (1 << (shift-1))) >> shift, cv2.cvtColor(BGR2GRAY) on uint8 [external: restated, not linked;
 * OpenCV 3: 1868, 9617, 4899, 14; OpenCV 4: 3735, 19235, 9798, 15]; skipped for C = 1.  Then PIL.Image.resize((rw, rh), BILINEAR):
 * horizontal pass (skipped when rw == sw), rounded and clipped to 8 bits, vertical pass (skipped when rh == sh); per axis scale =
 * in/out, support = max(scale, 1), ksize = (int)ceil(support)*2 + 1, output i reads source samples xmin .. xmin + n with
 * xmin = max((int)(center - support + 0.5), 0), xmin + n = min((int)(center + support + 0.5), in), center = (i + 0.5)*scale, with the
 * normalised triangle weights in 22-bit fixed point: pixel = clip((2^21 + sum src*kk) >> 22, 0, 255).  Only the window of H x W
 * outputs at (dy, dx) of the (rh, rw) resize is evaluated (cvt_img2train's crop_rate branch resizes, then crops).  The result goes
 * through lut256_dev, 256 floats made by the host as float32(float64(u) * (1./255) - 0.5) -- what TensorFlow is fed -- to out
 * float32 [N,H,W].  Two launches: rows (grey + horizontal, the source row in LDS) into the workspace uint8 [N][rows needed][W], then
 * columns + table.  The horizontal tap count is bounded by the LDS tile: ksize <= 8193 (a 4096x downscale), refused before the
 * first launch otherwise; the vertical one is not bounded.
 * Colour: cv2.resize(img, (W, H)), INTER_LINEAR, uint8 [external]: per axis f = (float)((d + 0.5)*src/dst - 0.5), s = floor(f), the
 * taps s and min(s+1, src-1) with short(rint((1-f)*2048)), short(rint(f*2048)) (f = 0 at a clamped edge); horizontal sums S in int32,
 * out = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.  One launch, out uint8 [N,H,W,3].
 * Nothing allocates, synchronises or copies from the host inside stabnet_ingest_grey / _colour. */
/* host; Pillow's taps of one axis: *ksize, bounds2 [out][2] = (xmin, n), kk [out][ksize] (cap = ints kk can take).  Returns
 * out * ksize (with bounds2 and kk NULL: only that, and *ksize if given), -1 on bad arguments or a cap too small. */
int stabnet_ingest_pil_taps(int in, int out, int* ksize, int* bounds2, int* kk, int cap);
/* host; cv2's taps of one axis: ofs2 [dst][2] source indices, coef2 [dst][2] weights of 2048. */
int stabnet_ingest_cv_taps(int src, int dst, int* ofs2, short* coef2);
size_t stabnet_ingest_workspace_bytes(int N, int sh, int sw, int C, int rh, int rw, int H, int W);    /* for any window origin; 0 = bad arguments */
/* x*_dev / y*_dev: what stabnet_ingest_pil_taps gives for (sw, rw) / (sh, rh), ON THE DEVICE (NULL allowed for a skipped pass). */
int stabnet_ingest_grey(const unsigned char* img, int N, int sh, int sw, int C, size_t row_stride_bytes, int wb, int wg, int wr,
                        int shift, int rh, int rw, int dy, int dx, int H, int W, const int* xbounds_dev, const int* xkk_dev, int xksize,
                        const int* ybounds_dev, const int* ykk_dev, int yksize, const float* lut256_dev, float* out, void* workspace,
                        size_t workspace_bytes, void* stream, void* prof);
/* x*_dev / y*_dev: what stabnet_ingest_cv_taps gives for (sw, W) / (sh, H), ON THE DEVICE.  C must be 3. */
int stabnet_ingest_colour(const unsigned char* img, int N, int sh, int sw, int C, size_t row_stride_bytes, int H, int W,
                          const int* xofs_dev, const short* xcoef_dev, const int* yofs_dev, const short* ycoef_dev, unsigned char* out,
                          void* stream, void* prof);

/* ---- behind the decoder, in front of the augmentation: the reference's get_img (get_data_mini_after.py:149-156) ----
 * Decoded uint8 BGR frames to channels of a training tensor dst float32 [N,H,W,C], one launch per destination tensor:
 * tf.image.rgb_to_grayscale, convert_image_dtype(float32), resize_images(method=0), - 0.5 with TensorFlow 1.3's arithmetic
 * [external: restated, not linked]: c = float(u8) * float(1/255); s = (r*0.2989f + g*0.5870f) + b*0.1140f, summed left to right,
 * every operation rounded to float32, no fused multiply-add; u = uint8(trunc(s * 255.5f)); f = float(u) * float(1/255); the legacy
 * bilinear resize (align_corners = False, no half-pixel centres): scale = float(in)/float(out), in_y = float(y)*scale,
 * top = floor(in_y), bottom = in_y < in-1 ? ceil(in_y) : in-1, lerp = in_y - floor(in_y), t = tl + (tr-tl)*xl, b = bl + (br-bl)*xl,
 * out = t + (b-t)*yl; then - 0.5f.
 * table_dev: int64 [n_entries][6] ON THE DEVICE = (byte offset of the frame from frames_u8, sh, sw, row stride in bytes, n, c):
 * the frame (pixels B, G, R, dense; rows strided) that fills dst[n, :, :, c].  One frame may be named by several entries, the
 * frames of one launch may differ in size.  When two entries name the same (n, c) the later one counts.  An entry whose frame does
 * not lie inside [frames_u8, frames_u8 + frames_bytes) (or sh, sw > 65536, stride < 3*sw) or whose (n, c) lies outside dst is not
 * followed: nothing is read or written out of bounds whatever the table holds.  A channel (n, c) that no entry names keeps what it
 * held.  C <= 32.  One launch, organised by destination (a workgroup owns 256 consecutive pixels of one n and stores them as dense
 * rows of C floats); no atomics, no workspace, nothing allocates, synchronises or copies from the host: capturable in a hipGraph. */
int stabnet_tf_get_img(const unsigned char* frames_u8, size_t frames_bytes, const int64_t* table_dev, int n_entries, float* dst, int N,
                       int H, int W, int C, void* stream, void* prof);

/* ---- beside the dataset: TV-L1 optical flow, to fill the records' flow (csrc/tvl1.hip; tests/tvl1_model.py is the yardstick) ----
 * Zach / Pock / Bischof TV-L1 in the IPOL formulation [external: restated from the paper, nothing linked], cut down to deterministic
 * float32 stencils: a FIXED number of inner iterations (no epsilon stop), no median filter, bilinear warps, pyramid factor 2.
 * i0, i1: float32 [B,H,W] on the 0..255 scale, pixels pixel_stride floats apart, rows W*pixel_stride, images H*W*pixel_stride (a
 * channel of an NHWC tensor is read in place).  stabnet_tvl1_flow reads (v + in_offset) * in_scale, two rounded operations (0, 1: v
 * itself; 0.5, 255: a get_img channel to the 0..255 scale), the stage entry points v itself.  The flow u = (u1, u2) in pixels satisfies i1(x + u1, y + u2) ~ i0(x, y).
 * Levels: one more while there are fewer than `scales` and min(h, w) / 2 >= min_side; one level down = [1,4,6,4,1]/16 along x,
 * then along y, replicated borders, then the pixels at even (y, x).  Per level, coarse to fine: u = 2 * upsample(u) (half-pixel
 * centred bilinear, source (i + 0.5)*0.5 - 0.5, clamped) or 0; the duals p11, p12, p21, p22 = 0; I1x, I1y = 0.5*(next - prev) on
 * replicated borders.  Per warp: Ix, Iy, Iw = I1x, I1y, I1 sampled bilinearly at (x + u1, y + u2), coordinates clamped to
 * [0, n-1], upper neighbour clamped to n-1; g = Ix*Ix + Iy*Iy; rc = ((Iw - Ix*u1) - Iy*u2) - I0.  Per iteration, with
 * lt = lambda*theta and taut = tau/theta (float32): rho = (rc + Ix*u1) + Iy*u2; f = lt if rho < -lt*g, -lt if rho > lt*g, -rho/g if
 * g > 1e-10f, else 0; u = (u + f*(Ix, Iy)) + theta*div(p), div = backward differences (first column / row: p itself, last: -p[x-1]);
 * p = (p + taut*grad u) / (1 + taut*sqrt(ux*ux + uy*uy)) per component, grad = forward differences (zero in the last column / row).
 * Every operation is one float32 operation, rounded once, in this order.  Non-finite pixel values are the caller's error: nothing
 * is read or written out of bounds for them, but the flow they give is unspecified.
 * Planes: u [2][B][H][W] = u1, u2; state [6][B][H][W] = u1, u2, p11, p12, p21, p22; consts [4][B][H][W] = Ix, Iy, rc, g.
 * stabnet_tvl1_iterate runs n iterations on `state` in place (`scratch` is a second buffer of the same size: a sweep cannot run in
 * place); fused = 0: one launch per iteration; fused = 1: up to K iterations per launch by temporal blocking in LDS and registers
 * (stabnet_tvl1_fused_geometry gives K and the tile).  Both write the same bits.
 * stabnet_tvl1_flow is the whole solve: uv_out [B,H,W,2] in pixels and / or map_out [B,H,W,2] in the convention interpolate() reads
 * (xp = (x + 1)*W/2): map[..., 0] = 2*(j + u1)/W - 1, map[..., 1] = 2*(i + u2)/H - 1; either may be NULL.  It takes the fused
 * iteration unless the environment holds STABNET_TVL1_FUSED=0.  workspace: stabnet_tvl1_workspace_bytes, 16-byte aligned.  Nothing
 * allocates, synchronises, reads back or copies from the host; no atomics; every launch goes to `stream`: capturable in a hipGraph.
 * Bad arguments (-1, before anything touches the GPU): null pointers, B < 1, H or W < 8 (stage entry points: < 2), a workspace too
 * small, tau / lambda / theta not positive, scales / warps / iters < 1, min_side < 2, more than 2^31 - 1 floats per tensor. */
int stabnet_tvl1_levels(int H, int W, int scales, int min_side, int* hw);     /* host; the number of levels, hw [levels][2] (or NULL); -1 */
void stabnet_tvl1_fused_geometry(int* k_tx_ty);                              /* host; K, tile width, tile height of the fused kernel */
size_t stabnet_tvl1_workspace_bytes(int B, int H, int W, int scales, int min_side);                /* host; 0 = bad arguments */
int stabnet_tvl1_pyramid_down(const float* in, int pixel_stride, int B, int H, int W, float* out, void* stream, void* prof);
int stabnet_tvl1_gradient(const float* in, int pixel_stride, int B, int H, int W, float* gx, float* gy, void* stream, void* prof);
int stabnet_tvl1_warp(const float* i0, const float* i1, int pixel_stride, const float* gx, const float* gy, const float* u, float* consts,
                      int B, int H, int W, void* stream, void* prof);
int stabnet_tvl1_upsample(const float* u_coarse, int B, int h, int w, float* u_fine, int H, int W, void* stream, void* prof);
int stabnet_tvl1_flow_to_map(const float* u, int B, int H, int W, float* uv_out, float* map_out, void* stream, void* prof);
int stabnet_tvl1_iterate(float* state, float* scratch, const float* consts, int B, int H, int W, float tau, float lambda, float theta, int n,
                         int fused, void* stream, void* prof);
int stabnet_tvl1_flow(const float* i0, const float* i1, int pixel_stride, float in_offset, float in_scale, int B, int H, int W, float tau, float lambda, float theta,
                      int scales, int warps, int iters, int min_side, void* workspace, size_t workspace_bytes, float* uv_out,
                      float* map_out, void* stream, void* prof);

/* ---- beside the dataset: corner tracking, to fill the records' feature_matches1 / 2 (csrc/klt.hip; tests/klt_model.py is the yardstick) ----
 * Shi-Tomasi corners, one per grid cell, tracked by pyramidal Lucas-Kanade with a FIXED number of iterations (no early stop) and kept
 * when the track back returns to the start [external: restated from the papers of Shi / Tomasi and Bouguet, nothing linked].
 * i0 (the stable frame), i1 (the unstable frame of the same instant): float32 [B,H,W], pixels pixel_stride0 / pixel_stride1 floats
 * apart (rows W*stride, images H*W*stride: a channel of an NHWC tensor is read in place), read as (v + in_offset) * in_scale, two
 * rounded operations, which must give the 0..255 scale (0, 1: v itself).  Every operation is one float32 operation, rounded once, in
 * this order; sqrt and / are the correctly rounded ones.
 * 1 Pyramids of both images: TV-L1's (above), one more level while there are fewer than `levels` and min(h, w) / 2 >= min_side.
 * 2 Response on level 0 of i0: gx, gy = 0.5*(next - prev); a, b, c = the sums of gx*gx, gx*gy, gy*gy over the (2r+1)^2 box, first
 *   along x from left to right, then along y from top to bottom; resp = 0.5*((a + c) - sqrt((a - c)*(a - c) + 4*(b*b))); resp = 0
 *   for pixels closer than `border` to an image edge (border >= r + 1: no box leaves the image).
 * 3 One candidate per cell x cell pixels (row-major cells; partial cells at the right and bottom edges count): the largest
 *   response, ties to the smallest (y, x).  detected = resp > 0 and resp >= floor and resp >= quality * (the image's largest resp).
 * 4 Track p from image A to image B, coarse to fine, d = 0 at the coarsest level; at level l, p_l = p * 2^-l: window sample s in
 *   [0, (2R+1)^2) has the offset o = (s mod (2R+1) - R, s div (2R+1) - R) and lies at (x, y) = p_l + o; T, Tx, Ty = A's level and its
 *   gradient planes sampled bilinearly there (coordinates clamped to [0, n-1], the upper neighbour to n-1, a NaN coordinate reads 0).
 *   A window sum of v[s]: lane j of a 64-lane wave starts from 0 and adds v[j], v[j+64], v[j+128], v[j+192] (those below (2R+1)^2)
 *   in this order; then six steps with partner distances 32, 16, 8, 4, 2, 1, each v = v + the partner's v.
 *   a, b, c = the window sums of Tx*Tx, Tx*Ty, Ty*Ty; det = a*c - b*b; lost when 0.5*((a+c) - sqrt((a-c)*(a-c) + 4*(b*b))) / (2R+1)^2
 *   < min_eig or det == 0.  Exactly `iters` times: e = T - B_l(y + d.y, x + d.x); bx, by = the window sums of e*Tx, e*Ty;
 *   d.x = d.x + (c*bx - b*by)/det; d.y = d.y + (a*by - b*bx)/det.  Then q_l = p_l + d; lost unless 0 <= q_l.x <= w-1 and
 *   0 <= q_l.y <= h-1 (a non-finite q_l is lost); d = 2*d for the next finer level.  A lost point stays lost; its arithmetic goes on.
 * 5 q = the forward track of p from i0 to i1; p' = the track of q from i1 to i0; fb2 = (p'.x - p.x)^2 + (p'.y - p.y)^2.  A match is
 *   valid when it was detected, neither track lost it and fb2 <= fb*fb.
 * 6 The row of a valid match: (2*p.x)/W - 1, (2*p.y)/H - 1, (2*q.x)/W - 1, (2*q.y)/H - 1; rows in cell order.  The reference wants the
 *   count to be smaller than max_matches, so at most max_matches - 1 rows are kept, the first in cell order; every row from n on is 0.
 * cand [B][cells][4] = x, y, resp, detected (1 / 0); trk [B][N][4] = q.x, q.y, lost (1 / 0), fb2, a lost point's row being 0, 0, 1, 0;
 * pts [B][N][2] = x, y; matches [B][max_matches][4]; n [B] int32.  stabnet_klt_response / _detect / _track are the stages alone
 * (_track builds the pyramids into the workspace first); stabnet_klt_matches is the whole solve: detection, one tracking launch (one
 * wave per cell, both directions) and one finishing launch.  workspace: stabnet_klt_workspace_bytes (for _track that of any cell
 * size), 16-byte aligned, as are cand, trk and matches.  Nothing allocates, synchronises, reads back or copies from the host; no
 * atomics; every launch goes to `stream`: capturable in a hipGraph.
 * Bad arguments (-1, before anything touches the GPU): null pointers, B < 1, H or W < 2*border + 1 (_track: < 3), border < r + 1, r
 * outside 1..4, cell < 2, max_matches < 2, a workspace too small, floor / quality / fb / iters not positive, levels outside 1..8,
 * min_side < 2, R outside 1..7 (a lane owns four window samples), min_eig negative, more than 2^31 - 1 floats per tensor. */
int stabnet_klt_cells(int H, int W, int cell, int* rows_cols);                 /* host; the number of cells, rows_cols [2] (or NULL); -1 */
size_t stabnet_klt_workspace_bytes(int B, int H, int W, int levels, int min_side, int cell);        /* host; 0 = bad arguments */
int stabnet_klt_response(const float* i0, int pixel_stride, float in_offset, float in_scale, int B, int H, int W, int r, int border, float* resp,
                         void* stream, void* prof);
int stabnet_klt_detect(const float* i0, int pixel_stride, float in_offset, float in_scale, int B, int H, int W, int r, int border, int cell,
                       float floor, float quality, float* cand, void* stream, void* prof);
int stabnet_klt_track(const float* i0, const float* i1, int pixel_stride0, int pixel_stride1, float in_offset, float in_scale, int B, int H, int W,
                      const float* pts, int N, int levels, int min_side, int R, int iters, float min_eig, void* workspace, size_t workspace_bytes,
                      float* trk, void* stream, void* prof);
int stabnet_klt_matches(const float* i0, const float* i1, int pixel_stride0, int pixel_stride1, float in_offset, float in_scale, int B, int H, int W,
                        int levels, int min_side, int r, int border, int cell, float floor, float quality, int R, int iters, float min_eig, float fb,
                        int max_matches, void* workspace, size_t workspace_bytes, float* matches, int* n, void* stream, void* prof);

/* ---- beside the matches: a robust homography per pair, for scoring a stabilised clip (csrc/homfit.hip; tests/homfit_model.py is the yardstick) ----
 * RANSAC with a fixed number of four-point hypotheses, a least-squares refit over the winner's inliers, the final inlier mask
 * [external: restated from Fischler / Bolles 1981 and Heckbert's projective mapping through the unit square, nothing linked].
 * matches [B][M][4] float32 and n [B] int32 as stabnet_klt_matches writes them, on the device: a row is (x0, y0, x1, y1) in the frame
 * 2x/W - 1, 2y/H - 1; only the first n[b] rows of pair b are read (n is clamped to 0..M), staged once in LDS.  One workgroup of 256
 * threads per pair.  float32 and float64 operations are single operations, rounded once, in this order; / and sqrt are the correctly
 * rounded ones; uint32 arithmetic wraps.
 * 1 mix(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16.  chain = mix(mix(seed + 0x9e3779b9) + b);
 *   base_k = mix(chain + k); draw d = 0..15 of hypothesis k: j = (uint64(mix(base_k + d)) * n) >> 32, taken unless the sample holds
 *   j already or is complete.  A hypothesis with fewer than four indices after 16 draws is invalid.  Thread t owns k = t, t + 256, ...
 * 2 With the sample's rows i = 0..3 in the order drawn, p_i = (x0, y0) and q_i = (x1, y1):  adj(p) = the rows
 *   (y1-y2, x2-x1, x1*y2 - x2*y1), (y2-y0, x0-x2, x2*y0 - x0*y2), (y0-y1, x1-x0, x0*y1 - x1*y0) of p_0..2; lambda_i = (adj_i0*x3 +
 *   adj_i1*y3) + adj_i2; mu_i the same from q;  s_0 = mu_0*(lambda_1*lambda_2), s_1 = mu_1*(lambda_0*lambda_2), s_2 = mu_2*(lambda_0*
 *   lambda_1);  t_0i = q_i.x*s_i, t_1i = q_i.y*s_i, t_2i = s_i;  G_rc = (t_r0*adj(p)_0c + t_r1*adj(p)_1c) + t_r2*adj(p)_2c;
 *   h_0..7 = G_0..7 / G_8.  Invalid when any of the eight is not finite.
 * 3 Row i < n is an inlier of h when w = (h6*x0 + h7*y0) + 1 > w_min and ((u/w - x1)*(W/2))^2 + ((v/w - y1)*(H/2))^2 <= thr_px*thr_px,
 *   u = (h0*x0 + h1*y0) + h2, v = (h3*x0 + h4*y0) + h5.  The best hypothesis is the valid one with the most inliers, ties to the smallest k.
 *   n < 4, no valid hypothesis, or fewer than max(4, min_inliers) inliers: status 0, Hm and mask all 0, count 0, best -1.
 * 4 Refit in float64 over the best hypothesis's inliers: the normal equations of the rows (x, y, 1, 0, 0, 0, -u*x, -u*y | u) and
 *   (0, 0, 0, x, y, 1, -v*x, -v*y | v), (x, y, u, v) = the row.  Their 36 + 8 entries are 23 distinct sums (the others repeat one or are 0):
 *   S0..5 = x*x, x*y, x, y*y, y, 1;  S6..11 = (u*x)*x, (u*x)*y, u*x, (u*y)*y, u*y, u;  S12..17 = the same with v;  S18..22 = q*(x*x),
 *   q*(x*y), q*(y*y), q*x, q*y with q = u*u + v*v.  Thread t adds its inlier rows t, t + 256, ... in order from 0; six steps with partner
 *   distances 32, 16, 8, 4, 2, 1 inside each 64-lane wave, each S = S + the partner's S; then ((wave 0 + wave 1) + wave 2) + wave 3.
 *   Lower triangle: A00 A10 A11 A20 A21 A22 = S0 S1 S3 S2 S4 S5, again for A33..A55; A6. = -S6 -S7 -S8 -S12 -S13 -S14 S18;
 *   A7. = -S7 -S9 -S10 -S13 -S15 -S16 S19 S20; b = S8 S10 S11 S14 S16 S17 -S21 -S22.  Cholesky column by column: d = Ajj - sum_k<j
 *   Ljk*Ljk (k ascending, one subtraction each), Ljj = sqrt(d), Lij = (Aij - sum_k<j Lik*Ljk) / Ljj; then L z = b and L^T h = z the
 *   same way (k ascending).  A d that is not > 0, or a solution that is not finite after its one rounding to float32, keeps the
 *   hypothesis: status 2; else status 1.
 * 5 mask and count: step 3's test under the final Hm (h33 = 1); mask is 0 from row n on.
 * Hm [B][9] float32, mask [B][M] uint8, count, status, best [B] int32, all on the device.  No workspace, no atomics, no allocation,
 * nothing synchronises, reads back or copies from the host; one launch on `stream`: capturable in a hipGraph.
 * Bad arguments (-1, before anything touches the GPU): null pointers, B outside 1..65535, M outside 4..1024 (16 KiB of LDS), H or W
 * outside 1..2^20, hypotheses outside 1..65536, thr_px not positive and finite, min_inliers < 0, seed < 0, w_min negative or not
 * finite, matches not 16-byte aligned. */
int stabnet_homfit(const float* matches, const int* n, int B, int M, int H, int W, int hypotheses, float thr_px, int min_inliers, int seed,
                   float w_min, float* Hm, unsigned char* mask, int* count, int* status, int* best, void* stream, void* prof);

/* ---- full-frame output: uncovered pixels filled from earlier stabilised frames (csrc/mosaic.hip; tests/mosaic_model.py is the yardstick) ----
 * [external: the mosaicking step of full-frame stabilisation as the literature describes it, Matsushita et al. 2006 among others,
 * restated with one global homography; nothing linked.]  float32 and float64 operations are single operations, rounded once, in
 * this order; everything else is integer arithmetic.
 *
 * stabnet_mosaic_guard_matches: keep only the matches that lie on content.  matches [B][M][4] float32 and n [B] int32 as
 * stabnet_klt_matches writes them (only the first n[b] rows are read, n clamped to 0..M); black0, black1 [B][H][W] float32: the
 * network's `black` of the frame each end of a row lives in ((x0, y0): black0; (x1, y1): black1).  An end (xn, yn) is SAFE when, with
 * X = ((xn + 1)*W)*0.5 and Y = ((yn + 1)*H)*0.5 in float32, xr = rintf(X), yr = rintf(Y) (half to even), g = guard:
 * xr - g >= 0, xr + g <= W - 1, yr - g >= 0, yr + g <= H - 1 (float32; all false for a NaN) and black[yr + dy][xr + dx] < 0.5 for
 * every |dx|, |dy| <= g (a NaN black is not < 0.5).  Row r < n[b] is kept when both ends are safe; the kept rows go to out_matches
 * [B][M][4] in their order, zeros from row out_n[b] on; out_n [B] int32.  One workgroup of 1024 threads per pair, a row per thread,
 * positions from wave ballots and sixteen LDS slots: no atomics, no workspace, nothing allocates, synchronises or reads back;
 * one launch on `stream`, capturable in a hipGraph.
 * Bad arguments (-1, before anything touches the GPU): null pointers, out_matches == matches, B outside 1..65535, M outside 4..1024,
 * guard outside 0..16, H or W outside 1..2^20, matches or out_matches not 16-byte aligned.
 *
 * stabnet_mosaic_compose: one launch per frame over [N][SH][SW] output pixels, uint8 BGR.  warped [N][SH][SW][3], px, py float32
 * [N][SH][SW]: out, px_out, py_out of stabnet_warp_rev_bundle2_src for this frame; canvas_prev [N][SH][SW][3] and age_prev uint8
 * [N][SH][SW]: the previous call's canvas_cur, age_cur (age 255: the pixel holds nothing); Hm [N][9] float32 and status [N] int32 as
 * stabnet_homfit writes them for matches tracked from frame t (i0) into frame t - 1 (i1), both read WHEN THE KERNEL RUNS: a captured
 * graph replays with what an earlier launch on the stream wrote.  H, W: the network's size (the frame Hm lives in).
 * Per pixel (i, j) of stream n, F = 32 << feather_log2:
 * 1 q(p) of a float32 p: t = fmin(fmax(p*32, -2e9), 2e9), rintf(t) as int32, -2e9 for a NaN (the remap's quantisation to 1/32 px).
 *   qx = q(px), qy = q(py); d = min(qx, 32*(SW-1) - qx, qy, 32*(SH-1) - qy); covered = d >= 0 (the remap's own coverage rule);
 *   a = min(max(d, 0), F).
 * 2 d >= F: out = warped, age = 0, counted fresh; nothing else is read.
 * 3 Otherwise the history sample; unavailable at once unless status[n] is 1 or 2.  In float64, h = Hm[n] widened:
 *   ax = 2/SW, cx = (1/SW - 1/W) - 1, ay = 2/SH, cy = (1/SH - 1/H) - 1       (A: x_n = ax*j + cx, cv2's half-pixel convention between
 *   sx = 0.5*SW, tx = (0.5*SW + (0.5*SW)/W) - 0.5, sy, ty alike with SH, H    SW and W pixels, then 2u/W - 1; B: j = sx*x_n + tx)
 *   m = h A: m[3r] = h[3r]*ax, m[3r+1] = h[3r+1]*ay, m[3r+2] = (h[3r]*cx + h[3r+1]*cy) + h[3r+2], r = 0..2;
 *   G = B m: G[c] = sx*m[c] + tx*m[6+c], G[3+c] = sy*m[3+c] + ty*m[6+c], G[6+c] = m[6+c], c = 0..2;
 *   u = (G0*j + G1*i) + G2, v = (G3*j + G4*i) + G5, w = (G6*j + G7*i) + G8; unavailable unless w > (double)w_min (false for a NaN);
 *   qx = q64(u/w), qy = q64(v/w), q64 being q in float64 (fmin, fmax, rint, int32).  ix = qx >> 5, fx = qx & 31, iy, fy alike; the
 *   taps (iy, ix), (iy, ix+1), (iy+1, ix), (iy+1, ix+1) of canvas_prev have the weights (32-fy)*(32-fx), (32-fy)*fx, fy*(32-fx),
 *   fy*fx (sum 1024; no table quirk); a tap COUNTS when its weight is not 0.  Available when every counting tap lies inside the
 *   frame and has age_prev < 255 and hist_age = 1 + (the largest age_prev of the counting taps) <= max_age.
 *   hist_c = (sum of value*weight + 512) >> 10 per channel (a tap that does not count adds nothing).
 * 4 covered, available:   out_c = (warped_c*a + hist_c*(F - a) + F/2) >> (5 + feather_log2); age = 0 when 2*a >= F, else hist_age; blended
 *   uncovered, available: out = hist, age = hist_age; history.     covered, unavailable: out = warped, age = 0; fresh.
 *   uncovered, unavailable: out = 0, age = 255; empty.
 * canvas_cur [N][SH][SW][3], age_cur [N][SH][SW]; counts [N][4] int32 += {fresh, blended, history, empty} of the frame (the caller
 * zeroes it on the stream; integer atomics after a wave / LDS sum, a workgroup covering several rows and adding two counters with
 * one 64-bit add where counts is 8-byte aligned: any order gives the same sums).
 * Two kernels with the same results: four pixels per thread (three dwords and two float4 in, three dwords and one age dword out)
 * when SW % 4 == 0, warped, canvas_cur, age_cur are 4-byte and px, py 16-byte aligned; one pixel per thread otherwise.  History taps
 * are read as six contiguous bytes per row; nothing outside a stream's own canvas is read.  Nothing allocates, synchronises or reads
 * back; one launch on `stream`, capturable in a hipGraph.
 * Bad arguments (-1, before anything touches the GPU): null pointers, N outside 1..65535, SH or SW outside 1..32767, H or W outside
 * 1..2^20, feather_log2 outside 0..6, max_age outside 1..254, w_min negative or not finite, canvas_cur == canvas_prev or
 * age_cur == age_prev. */
int stabnet_mosaic_guard_matches(const float* matches, const int* n, const float* black0, const float* black1, int B, int M, int H, int W,
                                 int guard, float* out_matches, int* out_n, void* stream);
int stabnet_mosaic_compose(const unsigned char* warped, const float* px, const float* py, const unsigned char* canvas_prev,
                           const unsigned char* age_prev, const float* Hm, const int* status, int N, int SH, int SW, int H, int W,
                           int feather_log2, int max_age, float w_min, unsigned char* canvas_cur, unsigned char* age_cur, int* counts,
                           void* stream);

/* ---- scene cuts (csrc/scene.hip) --------------------------------------------------------------------------
 * The online loop is recurrent: every frame is regressed against a ring of earlier STABILISED frames.  After a cut those hold
 * another scene.  These entries decide on the device, inside the frame's graph, whether the incoming grey frame starts a new scene,
 * and re-seed the ring when it does -- no host round trip, fixed arguments, capturable in a hipGraph.
 *
 * The statistic is all integers, so any grid shape and any order of the atomics gives the same bits.  For a train-normalised grey
 * frame g [N][H][W], float32 in [-0.5, 0.5]:
 *   t = floorf((g + 0.5f) * 255.0f + 0.5f), each operation one float32 rounding (no FMA contraction);
 *   t = fminf(fmaxf(t, 0.f), 255.f): a NaN lands in 0, -inf in 0, +inf in 255;
 *   q = (int)t, bin = q >> 3 (32 bins);  tile = (4*y / H) * 4 + (4*x / W), integer division: a 4 x 4 grid, ragged when H or W is
 *   no multiple of 4;  hist[n][tile][bin] = uint32 count;  D[n] = sum over tiles and bins of |hist_cur - hist_prev| (<= 2*H*W);
 *   the distance is d = D / (2*H*W), in [0, 1].
 *
 * stabnet_scene_state_words() = 1026.  The per-stream state is uint32 [N][1026] = {seen, since, prev[16][32], cur[16][32]} in device
 * memory; all zeros is a fresh stream.  Between calls cur is zero: the call's second kernel moves it to prev and zeroes it, so that
 * the next call's histogram kernel adds into zeros without a memset the graph cannot see.  After a call, prev is the histogram of
 * the frame the call was given.
 *
 * stabnet_scene_update: two launches on `stream`.  (1) the histogram of grey into cur: a workgroup takes up to 2048 consecutive
 * pixels of one tile row, counts into private LDS histograms (4 tile columns x 32 bins, one copy per wave and group of eight lanes),
 * then adds its non-zero counters with integer atomicAdd; four pixels per load when W % 4 == 0 and grey is 16-byte aligned, one
 * otherwise, with the same counts.  (2) one workgroup per stream forms D and evaluates the rule
 *   seen == 0:  flag = 0, D = 0 (the first frame has nothing to differ from);
 *   otherwise:  flag = (since >= min_gap) && (D > thr_num);
 * then since = flag ? 0 : since + 1 and seen = seen + 1 (both saturating at 0xffffffff), prev = cur, cur = 0, flag[n] = flag,
 * dist[n] = D.  The host computes thr_num = floor(threshold * 2.0 * H * W) in double, threshold in (0, 1].  `since` counts the
 * frames since the last flag (or since the start), so flashes closer than min_gap frames to the last cut are not flagged.
 * Nothing allocates, synchronises or copies to the host.
 * Bad arguments (-1, before any launch): null pointers, N outside 1..65535, H or W outside 4..32767, min_gap < 0, pointers that are
 * not memory of the current device.
 *
 * stabnet_ring_reseed_if: for every stream s with flag[s] != 0 what stabnet_ring_init does for that stream -- all `depth` frame
 * slots become first_frame[s], all mask slots 0; a stream with flag[s] == 0 is not touched (its workgroups load the flag and
 * return).  The ring head is left alone: with all slots equal its value does not matter.  flag: DEVICE int32 [S], read when the
 * kernel runs (what stabnet_scene_update wrote earlier on the stream, also in a replayed graph).  A null flag is refused:
 * stabnet_ring_init is the unconditional form.
 *
 * What a cut means: called as scene_update(cur), ring_reseed_if(ring, cur, flag), deploy_frame(cur), a flagged frame c meets a ring
 * of 32 x frame c with zero masks and is then stabilised like any other frame -- the run from c on equals a fresh run on the clip
 * that starts at c with its first frame doubled, bit for bit. */
int stabnet_scene_state_words(void);
int stabnet_scene_update(const float* grey, int N, int H, int W, unsigned thr_num, int min_gap, unsigned* state, int* flag,
                         unsigned* dist, void* stream);
int stabnet_ring_reseed_if(float* frames_ring, float* masks_ring, const float* first_frame, int S, int depth, int H, int W,
                           const int* flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STABNET_HIP_H */
