/*
 * pvr_train.h — C-ABI of the trainable ResNet encoder of libpvr_hip.so: EmbeddingNet(..., train=True)
 * (reference src/embeddings.py:323-326 model.train() / requires_grad, :396-398 the forward that keeps its graph;
 * exposed as --train_embedding, src/arguments.py:19).
 *
 * Scope: the torchvision trunks resnet18 / resnet34 / resnet50 (arch PVR_ARCH_RESNET18 / _RESNET34 / _RESNET50), fp32 storage,
 * every product of a convolution, a data gradient or a weight gradient on the f32-input MFMA (the arithmetic of the PVR_F32
 * plan), one GPU.  BatchNorm runs on the statistics of the WHOLE batch of a forward (they cannot be chunked) or, after
 * pvr_trainer_set_bn_frozen, on its running statistics (frames independent: a step is a sum over passes).  After
 * pvr_trainer_set_wgrad_split16 the weight gradients alone run as exact-split products on the f16 matrix pipe; after
 * pvr_trainer_set_conv_split16 the forward convolutions and the data gradients of layer1 .. layer4 do (conv1's forward, BatchNorm
 * and the pools stay in fp32).  Both modes are off by default and independent of each other and of the BatchNorm mode.  After
 * pvr_trainer_set_train_from(stage) only layer<stage> .. layer4 train (partial fine-tuning): conv1 / bn1 and the layers below are a
 * frozen prefix that runs on its running statistics, keeps no activations and has no backward; its gradient span is zero.
 *
 * Buffers follow pvr_policy.h's convention: the caller owns ONE flat fp32 device buffer of parameters, every tensor in its
 * state_dict shape (conv weights in torch's (cout, cin, kh, kw) layout - the library repacks them inside the forward), and
 * steps it in place with any optimizer; the library reads it on the next forward.  A second flat buffer holds the BatchNorm
 * buffers.  Status codes, error messages and stream handling as in pvr_hip.h.
 */
#ifndef PVR_TRAIN_H
#define PVR_TRAIN_H

#include "pvr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pvr_trainer pvr_trainer;

/* desc as for pvr_encoder_create; arch RESNET50 / RESNET18 / RESNET34 with dtype PVR_F32, anything else is PVR_ERR_INVALID with a
 * message that names what is trainable; so is a max_batch at which one tensor of the workspace would pass 2 GiB (the launches address an operand
 * with 32-bit byte offsets: 668 frames for resnet18 / 34, 334 for resnet50; the message names the number).  Host arithmetic only: the workspace (one saved pre-BN and one post-BN tensor per
 * convolution, their gradients, the scratch of the split reductions - sized for max_batch frames) is made by the first forward. */
pvr_status pvr_trainer_create(const pvr_encoder_desc *desc, pvr_trainer **out);
void pvr_trainer_destroy(pvr_trainer *tr);
int32_t pvr_trainer_out_size(const pvr_trainer *tr);

/* bytes of the device workspace the first forward will allocate for this handle's max_batch (host arithmetic only): what a caller compares
 * with the free device memory before it trains */
int64_t pvr_trainer_workspace_bytes(const pvr_trainer *tr);

/* the flat parameter buffer: its length in floats; name of tensor `index` in buffer order (returns the length, 0 past the end);
 * offset of a tensor by its state_dict name ("layer2.0.downsample.0.weight"), -1 if there is none - *numel and shape[0..3]
 * (unused dimensions 0) are filled when the pointers are given */
int64_t pvr_trainer_param_count(const pvr_trainer *tr);
int32_t pvr_trainer_param_name(const pvr_trainer *tr, int32_t index, char *buf, int32_t cap);
int64_t pvr_trainer_param_offset(const pvr_trainer *tr, const char *name, int64_t *numel, int64_t *shape);
/* the BatchNorm buffer block, counted in 4-byte slots: running_mean and running_var of every BatchNorm as fp32, then one int64
 * num_batches_tracked per BatchNorm (two slots each, 8-byte aligned).  offset by name ("bn1.running_var",
 * "layer1.0.bn2.num_batches_tracked"), -1 if there is none */
int64_t pvr_trainer_buffer_count(const pvr_trainer *tr);
int64_t pvr_trainer_buffer_offset(const pvr_trainer *tr, const char *name, int64_t *numel);

/* Training-mode forward of n <= max_batch uint8 (n,h,w,3) frames: the integer transforms and fp32 Normalize of the PVR_F32 plan,
 * then per convolution the raw-weight convolution, BatchNorm on batch statistics (biased variance, eps 1e-5) [+ residual] [ReLU],
 * max pool, average pool; row i of the result at out_dev + i * out_stride.  Updates running_mean / running_var (momentum 0.1,
 * unbiased variance) and num_batches_tracked in bn_buffers_dev, and keeps every activation for ONE pvr_trainer_backward. */
pvr_status pvr_trainer_forward(pvr_trainer *tr, const float *params_dev, void *bn_buffers_dev, const uint8_t *frames_dev, int32_t n, int32_t h, int32_t w,
                               float *out_dev, int64_t out_stride, void *hip_stream);
/* d(loss)/d(out) (row i at dout_dev + i * dout_stride) -> d(loss)/d(params) in grads_dev, laid out as params and fully
 * overwritten.  One backward per forward: without a forward whose activations are still held it returns PVR_ERR_STATE.
 * Bit-reproducible run to run (no float atomics: every split reduction is summed in a fixed order). */
pvr_status pvr_trainer_backward(pvr_trainer *tr, const float *params_dev, const float *dout_dev, int64_t dout_stride, float *grads_dev, void *hip_stream);

/* BatchNorm mode of the handle.  on == 0 (the default): batch statistics, everything above.  on != 0: FROZEN BatchNorm - the fine-tuning mode of a
 * pre-trained trunk (torch: model.train() followed by .eval() on every BatchNorm module): the convolutions and the BatchNorm affine parameters train,
 * BatchNorm normalises with running_mean / running_var (eps 1e-5) and pvr_trainer_forward leaves running_mean, running_var and
 * num_batches_tracked untouched.  Every frame is then independent of the others: a step over N frames is a sum over passes of <= max_batch frames
 * (pvr_trainer_backward_acc), the workspace is sized by the pass, and a pass of one frame is legal.  Switching drops a held forward (a following
 * backward is PVR_ERR_STATE). */
pvr_status pvr_trainer_set_bn_frozen(pvr_trainer *tr, int32_t on);
/* pvr_trainer_backward that can add to grads_dev.  accumulate == 0: pvr_trainer_backward (scratch unused).  accumulate != 0: this pass's gradient is
 * written to the caller's scratch_dev (scratch_floats >= pvr_trainer_param_count) and ONE launch adds it onto grads_dev, one fp32 addition per
 * element - the result of a step depends on the order of its passes and on nothing else.  Allowed in both BatchNorm modes; only with frozen
 * BatchNorm is the sum over passes the gradient of the whole batch.  The scratch is the caller's so that pvr_trainer_workspace_bytes does not
 * depend on how a caller steps. */
pvr_status pvr_trainer_backward_acc(pvr_trainer *tr, const float *params_dev, const float *dout_dev, int64_t dout_stride, float *grads_dev,
                                    int32_t accumulate, float *scratch_dev, int64_t scratch_floats, void *hip_stream);
/* Weight-gradient arithmetic of the handle.  on == 0 (the default): every weight gradient on the f32-input MFMA, everything above, bit for bit.
 * on != 0: every weight gradient, conv1's included, is an exact-split product on the f16 matrix pipe (pvr_op_conv_wgrad_split16 /
 * pvr_op_stem_wgrad_split16: per-tensor power-of-two scales, a = a_hi + 2^-11 a_lo in f16, three MFMAs per fragment pair, fp32 accumulation, the
 * same fixed-order double reduction).  The forward, the data gradients and BatchNorm are untouched, so embeddings, running statistics and the
 * BatchNorm gradients keep their bits; a convolution weight gradient moves by about 2^-22 relative.  Legal in both BatchNorm modes.  The mode
 * decides the workspace (one scale slot per saved tensor, the split kernels' scratch), so it must be chosen before the first forward makes it:
 * afterwards the call returns PVR_ERR_STATE with a message.  pvr_trainer_workspace_bytes reports the size of the current mode; off, it is
 * what it was without the mode, to the byte. */
pvr_status pvr_trainer_set_wgrad_split16(pvr_trainer *tr, int32_t on);

/* Forward and data-gradient arithmetic of the handle.  on == 0 (the default): every convolution and data gradient on the f32-input MFMA, everything
 * above, bit for bit, and the same workspace to the byte.  on != 0: every convolution of layer1 .. layer4 computes z = conv(x, W), and every data gradient
 * dx [+]= conv(dz or its zero-filled stride-2 grid, rot180(W) transposed), as an exact-split product on the f16 matrix pipe (pvr_op_conv_fwd_split16 /
 * pvr_op_conv_dgrad_split16): both operands times a per-tensor power of two (pvr_op_absmax_scale's rule, read on the device), a = a_hi + 2^-11 a_lo in
 * f16, three MFMAs per fragment pair, fp32 accumulation, the scales undone exactly in the epilogue.  An activation's scale is computed once per forward,
 * in the launch that also takes its first consumer's weight scale; the backward reuses it (with pvr_trainer_set_wgrad_split16 too: the saved
 * activations and dz are scaled once for both uses).  conv1's forward, BatchNorm in either mode, the pools and - unless wgrad_split16 is on - the
 * weight gradients stay in fp32.  Results move by about 2^-22 relative per product; two runs give the same bits.  Legal in both BatchNorm modes, with
 * or without wgrad_split16.  The mode adds scale slots to the workspace, so it must be chosen before the first forward makes it: afterwards the call
 * returns PVR_ERR_STATE with a message.  pvr_trainer_workspace_bytes reports the size of the current mode.  pvr_trainer_launch_time names the mode's
 * launches: in the forward "<conv> scale" (weights [+ input]) and "<conv> split16" (weight pack + convolution), in the backward "<conv> bwd scale"
 * (dz + weights) and "<conv> dgrad split16" (weight pack [+ grid] + convolution). */
pvr_status pvr_trainer_set_conv_split16(pvr_trainer *tr, int32_t on);

/* Partial fine-tuning: the stage the handle trains from.  stage == 0 (the default): everything trains, everything above, bit for bit, and the same
 * workspace to the byte.  stage 1 .. 4: layer<stage> .. layer4 train; conv1 / bn1 and every layer below layer<stage> are the FROZEN PREFIX (torch:
 * those modules in .eval() with requires_grad = False).  Any other value is PVR_ERR_INVALID.
 *   forward: BatchNorm of every prefix op normalises with its running statistics whatever the handle's BatchNorm mode is, and reads its buffers only;
 *     in batch-statistics mode only the trained stages use and update batch statistics.  No prefix tensor is kept but the one a trained op reads (the
 *     boundary tensor: the last prefix output - for resnet18 / 34 at stage 1 the max pool's output, which is also layer1.0's residual): the prefix's
 *     tensors rotate through a small pool of buffers assigned by liveness, and a prefix op has no gradient tensor and no mean / rstd slots.  In the fp32
 *     arithmetic a prefix op of layer1 .. layer<stage-1> is ONE launch (pvr_op_conv_bn_frozen_forward: no pre-BN tensor exists); with conv_split16 on
 *     it is the mode's scale + split convolution followed by the frozen BatchNorm launch, because a mode has one arithmetic (one launch with the
 *     same bits after pvr_trainer_set_prefix_fused).  The stem stays conv1,
 *     bn1 and the max pool.
 *   backward: walks from the last op down to the first trained op and stops.  The ops that read the boundary tensor (the first block's conv1 and its
 *     downsample) compute their weight gradient and no data gradient; a residual that comes from the prefix gets no gradient; there is no max-pool
 *     backward, no bn1 backward and no conv1 weight gradient.  grads_dev stays fully overwritten: the span [0, pvr_trainer_trained_offset) is set to
 *     zero on the caller's stream (launch "prefix grads zero"); pvr_trainer_backward_acc adds those zeros like everything else.
 * The trained stages compute what they compute at stage 0: with frozen BatchNorm and conv_split16 (the prefix then runs the same launches as at
 * stage 0) the embeddings and every trained tensor's gradient keep their bits.  Legal in both BatchNorm modes and with either or both split modes.
 * The stage decides the workspace, so it must be chosen before the first forward makes it: afterwards a different stage is PVR_ERR_STATE with a
 * message.  pvr_trainer_workspace_bytes reports the size of the current stage. */
pvr_status pvr_trainer_set_train_from(pvr_trainer *tr, int32_t stage);
int32_t pvr_trainer_train_from(const pvr_trainer *tr);
/* float offset in the flat parameter buffer at which the trained parameters begin (0 at stage 0).  Parameters are laid out in op order, so the frozen
 * prefix is the one leading span [0, offset) and the offset is that of layer<stage>.0.conv1.weight. */
int64_t pvr_trainer_trained_offset(const pvr_trainer *tr);

/* The frozen prefix once per frame and step (the Python mode prefix_once).  With frozen BatchNorm a step runs as passes of <= max_batch frames and the
 * backward recomputes every pass but the last; the prefix (preprocess, normalize, conv1, bn1, max pool, every prefix op) is frozen, has no backward and
 * produces ONE tensor a trained op reads - the boundary tensor (the max pool's output, or the last prefix op's y).  A caller that keeps that tensor
 * across the passes of a step lets a recompute pass start at the first trained op.  The cache is the caller's, as pvr_trainer_backward_acc's scratch is:
 * pvr_trainer_workspace_bytes does not depend on how a caller steps, and the handle keeps no state about what the cache holds.
 * pvr_trainer_boundary_floats: floats per frame of the boundary tensor (host arithmetic; 0 at stage 0).  Per frame 56*56*64, 56*56*256, 28*28*512,
 *   14*14*1024 floats for resnet50 at stages 1 .. 4 and 56*56*64, 56*56*64, 28*28*128, 14*14*256 for resnet18 / 34.
 * pvr_trainer_forward_boundary, reuse == 0: pvr_trainer_forward, except that the launch that produces the boundary tensor of this pass writes it straight
 *   to boundary_dev (n x boundary_floats floats; nothing is copied) and the trained ops read it there.  reuse != 0: boundary_dev holds what an earlier
 *   reuse == 0 call wrote for these n frames; no preprocess, normalize, stem, pool or prefix launch runs, frames_dev may be null and the pass starts at the
 *   first trained op (pvr_trainer_launch_time lists nothing before it) - the same bits, because the trained ops read the same tensor.
 *   Either way the held forward remembers the pointer: its backward reads the boundary tensor there (the first block's weight gradients, the residual of
 *   resnet18's layer1.0, the split modes' scale of it), so the caller leaves that memory unchanged until the backward has run.  The whole cache of a step
 *   may pass 2 GiB: only the n frames of one call are an operand.  pvr_trainer_forward itself keeps using the workspace's own boundary piece.
 *   Refused by name, launching nothing: stage 0 (PVR_ERR_STATE: there is no prefix), a null or not 16-byte aligned boundary_dev, n outside
 *   1 .. max_batch, reuse == 0 with null frames. */
int64_t pvr_trainer_boundary_floats(const pvr_trainer *tr);
pvr_status pvr_trainer_forward_boundary(pvr_trainer *tr, const float *params_dev, void *bn_buffers_dev, const uint8_t *frames_dev, int32_t n, int32_t h,
                                        int32_t w, float *boundary_dev, int32_t reuse, float *out_dev, int64_t out_stride, void *hip_stream);
/* The split prefix op as one launch.  on == 0 (the default): everything above, bit for bit, and the same workspace to the byte.  on != 0, with
 * conv_split16 and a stage above 0: a prefix op is "<conv> scale" and "<conv> split16 bn frozen" (pvr_op_conv_bn_frozen_forward_split16: weight pack + the
 * split convolution with the frozen BatchNorm in its epilogue) instead of scale, split convolution and a BatchNorm launch; no pre-BN tensor of the prefix
 * exists, so the workspace shrinks.  The output keeps its bits.  Without conv_split16, or at stage 0, the mode changes nothing.  It decides the workspace,
 * so it must be chosen before the first forward makes it: afterwards the call returns PVR_ERR_STATE with a message.  pvr_trainer_workspace_bytes reports the
 * size of the current mode. */
pvr_status pvr_trainer_set_prefix_fused(pvr_trainer *tr, int32_t on);

/* The frozen prefix once per DATASET frame (the Python mode prefix_cache).  The prefix is frozen, runs on running statistics in either BatchNorm mode
 * and reads a frame behind a deterministic resize and centre crop: the boundary tensor of a frame is the same bits in every step.  A caller that holds
 * the dataset on the device computes every frame's boundary tensor once, before training (pvr_trainer_prefix_forward in blocks of <= max_batch frames
 * into one (N, boundary_floats) tensor of its own), and a training pass is then pvr_op_gather_rows of the pass's rows into a staging buffer followed by
 * pvr_trainer_forward_boundary(reuse != 0) on it.  The cache is the caller's and so is the rule of its validity: it holds what the prefix's
 * parameters and BatchNorm buffers gave when it was filled; the handle keeps no state about it.
 * pvr_trainer_prefix_forward: preprocess, normalize, conv1, bn1, the max pool and the prefix ops of n frames and nothing else - the launches
 *   pvr_trainer_forward_boundary(reuse == 0) runs before its first trained op (after pvr_trainer_set_prefix_fused the fused split launches), so the
 *   same bits; the launch that produces the boundary tensor writes it straight to boundary_dev (n x pvr_trainer_boundary_floats floats).  No trained op
 *   runs and no forward is held: a held forward is dropped (the call overwrites the stem's workspace) and a following pvr_trainer_backward is
 *   PVR_ERR_STATE.  pvr_trainer_launch_time lists exactly these launches.  Legal in both BatchNorm modes and with either split mode; the running
 *   statistics are read and never written.  Refused by name, launching nothing: stage 0 (PVR_ERR_STATE: there is no prefix), a null argument, a
 *   boundary_dev that is not 16-byte aligned, n outside 1 .. max_batch. */
pvr_status pvr_trainer_prefix_forward(pvr_trainer *tr, const float *params_dev, const void *bn_buffers_dev, const uint8_t *frames_dev, int32_t n, int32_t h,
                                      int32_t w, float *boundary_dev, void *hip_stream);
/* dst[i, :] = src[rows[i], :] for i < n: src (n_src_rows, row_floats) and dst (n, row_floats) fp32, rows n int64 indices on the device; all three in
 * device memory.  The gather of a cached pass, and the one new launch on its hot path: 16-byte lanes (row_floats % 4 == 0, both pointers 16-byte
 * aligned), a long row split over several workgroups (pieces of at most 16 KiB walked by a bounded grid, so that 2 rows of 3.2 MB and 334 rows of
 * 0.2 MB both fill the device).  Source offsets are 64-bit throughout: the source may pass 2 GiB, 4 GiB and 2^31 floats.  An index outside
 * [0, n_src_rows) is never dereferenced: its destination row is filled with quiet NaNs (0x7fc00000), so that a wrong index shows in the loss and cannot
 * fault.  Repeated indices are legal.  Plain vector loads and stores, no atomics: two runs give the same bits.  Refused by name, launching nothing: a
 * null argument, n < 1, n_src_rows < 1, row_floats < 4 or not a multiple of 4, a src_dev or dst_dev that is not 16-byte aligned or a rows_dev that is
 * not 8-byte aligned. */
pvr_status pvr_op_gather_rows(const float *src_dev, int64_t n_src_rows, int64_t row_floats, const int64_t *rows_dev, int64_t n, float *dst_dev,
                              void *hip_stream);

/* A random crop window per frame and step (the Python mode random_crop): the augmentation of fine-tuning on a few thousand small frames.  The centre crop
 * of every forward above becomes a window per frame, (top, left) in the RESIZED frame, chosen by the caller.
 * pvr_op_crop_windows / pvr_host_crop_windows: n windows, windows[2 i] = top in [0, max_top] and windows[2 i + 1] = left in [0, max_left] of frame
 *   first_frame + i, into device / host memory.  Frame f draws from Philox-4x32-10 with counter (f, call) and key seed (csrc/sample_rng.h):
 *   top = (bits0 * (max_top + 1)) >> 32 and left likewise from bits1 - uniform up to a relative bias below 2^-26 for ranges of at most 64 values.  Both
 *   functions share one inline and agree bit for bit.  The result depends on (seed, call, frame) alone - not on the grid and not on how a step is cut
 *   into passes: rows lo .. hi of one draw equal a draw with first_frame = lo.  torch's own generator stream is not reproduced; the contract is the
 *   distribution plus determinism.  The trainer's ranges are resized size - crop (32 x 32 for square frames).  pvr_op_crop_windows refuses by name,
 *   launching nothing: a null or not 4-byte aligned windows_dev, n < 1, a negative first_frame, max_top or max_left; the host function treats a negative
 *   maximum as 0 and writes nothing through a null pointer.
 * pvr_trainer_forward_windows, windows_dev == NULL: exactly pvr_trainer_forward (boundary_dev == NULL) or pvr_trainer_forward_boundary (given) - the
 *   same launches, names, bits and refusals.  windows_dev != NULL (n x (top, left) int32 on the device): the launches "preprocess" and "normalize" are
 *   replaced by ONE launch "preprocess windows" (pvr_op_preprocess_windows) that writes the fp32 image of each frame's window; everything after it is
 *   unchanged, and the held forward's image is the windowed one, so conv1's weight gradient sees it.  A window is clamped in the kernel to
 *   [0, resized height - crop] x [0, resized width - crop]: no value can make it read outside its frame.  Where the resize is exact arithmetic - no
 *   resize, and the power-of-two scales of 64 x 64 and 128 x 128 frames - the image has the bits the two launches give at that window; at other scales the
 *   new launch sums the taps in the rounding order of ATen's host kernel, so a .5 tie of the bilinear sum lands where torchvision's Resize puts it, which
 *   preprocess_kernel may miss by one uint8 step.  reuse != 0 (with boundary_dev): the pass starts at the first trained op, windows are not read and may be null.  The handle keeps
 *   nothing about windows: a recompute pass that runs the stem again is handed the same rows again.  pvr_trainer_prefix_forward keeps the centre crop - a
 *   cache of boundary tensors is only valid for a deterministic crop.  Refused by name, launching nothing: what pvr_trainer_forward_boundary refuses (a
 *   boundary_dev at stage 0, its alignment, n outside 1 .. max_batch, null frames without reuse), a windows_dev that is not 4-byte aligned, a frame whose
 *   resized size is below the crop. */
pvr_status pvr_op_crop_windows(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, int32_t max_top, int32_t max_left, int32_t *windows_dev,
                               void *hip_stream);
void pvr_host_crop_windows(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, int32_t max_top, int32_t max_left, int32_t *windows_host);
pvr_status pvr_trainer_forward_windows(pvr_trainer *tr, const float *params_dev, void *bn_buffers_dev, const uint8_t *frames_dev, int32_t n, int32_t h,
                                       int32_t w, const int32_t *windows_dev, float *boundary_dev, int32_t reuse, float *out_dev, int64_t out_stride,
                                       void *hip_stream);
/* The kernel of that launch alone: uint8 NHWC frames (n, h, w, 3) -> Resize(resize, bilinear, rounded to uint8 as torchvision does) -> the crop x crop
 * window at the clamped windows_dev[2 i], windows_dev[2 i + 1] of the resized frame -> (v / 255 - mean) / std per channel, channel 3 = 0 -> out_dev, the
 * dense fp32 NHWC4 image (n, crop, crop, 4), 16-byte aligned.  One 16-byte store per pixel, plain loads and stores, no atomics: two runs give the same
 * bits.  Refused by name, launching nothing: a null argument, a non-positive size, a resized frame smaller than the crop, a windows_dev that is not
 * 4-byte or an out_dev that is not 16-byte aligned, more than 65535 frames. */
pvr_status pvr_op_preprocess_windows(const uint8_t *frames_dev, int32_t n, int32_t h, int32_t w, int32_t resize, int32_t crop, const float *mean,
                                     const float *std_, const int32_t *windows_dev, float *out_dev, void *hip_stream);

/* Colour jitter per frame and step (the Python mode color_jitter): brightness, contrast and saturation as torchvision's ColorJitter applies them to a
 * uint8 tensor, without hue, on the uint8 values of each frame's crop x crop window - after Resize and the window, before / 255 and Normalize.
 * Arithmetic, every product and sum one fp32 rounding (no contraction):
 *   gray(r, g, b) = trunc(((0.2989f r) + (0.587f g)) + (0.114f b));   blend(a, b, f) = trunc(clamp((f a) + ((1.0f - f) b), 0, 255)) per channel;
 *   brightness f: blend(v, 0, f);   saturation f: blend(v, gray(v), f);   contrast f: blend(v, m, f) with m = (float)S / (float)(crop crop), S the INTEGER
 *   sum of gray over the frame's window of the image as it stands when contrast is applied.  S <= 255 * 256^2 < 2^24: (float)S is exact, m does not
 *   depend on the order of the sum, and the parallel reduction has the bits of torch.mean.  Factors (1, 1, 1) in any order reproduce the input bits.
 * A frame's parameters are four 32-bit words: float b, float c, float s, int32 order; order 0 .. 5 indexes the permutations of (brightness, contrast,
 *   saturation) in lexicographic order (0 = b c s, 1 = b s c, 2 = c b s, 3 = c s b, 4 = s b c, 5 = s c b).  Hardened in the kernels: a NaN factor counts
 *   as 1, a factor is clamped to [0, 4], an order outside 0 .. 5 counts as 0; no value can produce a NaN image.
 * pvr_op_color_params / pvr_host_color_params: the parameters of frames first_frame .. first_frame + n into device / host memory.  Frame f draws from
 *   Philox-4x32-10 with counter (f, call), as the crop windows do, and key (seed_lo, seed_hi ^ 0x434F4C52): a stream of its own, so the windows of the
 *   same (seed, call) keep their bits.  Words 0 .. 2: factor = fma(hi - lo, u, lo), u uniform in (0, 1), lo = max(0, 1 - strength), hi = 1 + strength
 *   (torchvision's range; strength 0 gives exactly 1); word 3: order = (bits * 6) >> 32.  Both functions share one inline (csrc/sample_rng.h) and agree
 *   bit for bit; the result depends on (seed, call, frame) alone: rows lo .. hi of one draw equal a draw with first_frame = lo.  pvr_op_color_params
 *   refuses by name, launching nothing: a null or not 4-byte aligned color_dev, n < 1, a negative first_frame, a negative or non-finite strength; the
 *   host function treats such a strength as 0 and writes nothing through a null pointer.
 * pvr_op_preprocess_color: pvr_op_preprocess_windows with the jitter between the window and / 255, as two launches: "colour stats" adds every frame's
 *   gray values before contrast into gray_sums_dev[i] (a wave reduction, then one integer atomicAdd per workgroup: no float atomics, two runs give the
 *   same bits), "preprocess colour" writes the image, one 16-byte store per pixel.  Both recompute the resized, windowed pixel with the expressions of
 *   pvr_op_preprocess_windows.  gray_sums_dev: n uint32 of the CALLER's scratch (pvr_trainer_workspace_bytes does not depend on how a caller steps); the
 *   entry point zeroes it on the stream before the stats launch (hipMemsetAsync), so it carries no state between calls.  The stats launch always runs:
 *   whether contrast is the identity is a fact of device data.  Refused by name, launching nothing: what pvr_op_preprocess_windows refuses, a null or not
 *   4-byte aligned color_dev or gray_sums_dev, a crop above 256.
 * pvr_trainer_forward_augmented, color_dev == NULL: exactly pvr_trainer_forward_windows - the same launches, names, bits and refusals.  color_dev != NULL
 *   needs windows_dev (without a random crop the caller passes the centre window, nearbyint((resized size - crop) / 2), for every frame): the two
 *   launches above replace "preprocess windows", everything after them is unchanged, and the held forward's image is the jittered one, so conv1's
 *   weight gradient sees it.  reuse != 0 (with boundary_dev): nothing before the first trained op runs and neither array is read.  The handle keeps
 *   nothing about the parameters: a recompute pass that runs the stem again is handed the same rows again.  pvr_trainer_prefix_forward keeps the plain
 *   centre crop.  Refused by name, launching nothing: what pvr_trainer_forward_windows refuses, a color_dev without windows_dev, a color_dev that is not
 *   4-byte aligned, a null or not 4-byte aligned gray_sums_dev. */
pvr_status pvr_op_color_params(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, float strength_b, float strength_c, float strength_s,
                               void *color_dev, void *hip_stream);
void pvr_host_color_params(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, float strength_b, float strength_c, float strength_s,
                           void *color_host);
pvr_status pvr_op_preprocess_color(const uint8_t *frames_dev, int32_t n, int32_t h, int32_t w, int32_t resize, int32_t crop, const float *mean,
                                   const float *std_, const int32_t *windows_dev, const void *color_dev, uint32_t *gray_sums_dev, float *out_dev,
                                   void *hip_stream);
pvr_status pvr_trainer_forward_augmented(pvr_trainer *tr, const float *params_dev, void *bn_buffers_dev, const uint8_t *frames_dev, int32_t n, int32_t h,
                                         int32_t w, const int32_t *windows_dev, const void *color_dev, uint32_t *gray_sums_dev, float *boundary_dev,
                                         int32_t reuse, float *out_dev, int64_t out_stride, void *hip_stream);

/* Random resized crop per frame and step (the Python mode random_resized_crop): torchvision's RandomResizedCrop(crop, scale = (lo, hi), ratio = (3/4, 4/3))
 * of the ORIGINAL uint8 frame - a rectangle of random area and aspect ratio, resized to crop x crop - in the place of Resize plus the window, before the
 * colour jitter, / 255 and Normalize.  A frame's rectangle is four int32: top, left, height, width, in the h x w frame.
 * pvr_op_crop_rects / pvr_host_crop_rects: the rectangles of frames first_frame .. first_frame + n into device / host memory (n x 4 int32), by
 *   get_params' rule.  Up to 10 tries; try t of frame f draws four words from Philox-4x32-10 with counter (f, call), as the windows do, and key (seed_lo,
 *   (seed_hi ^ 0x52454354) + t * 0x9E3779B9): a stream of its own, so pvr_op_crop_windows and pvr_op_color_params keep their bits at the same (seed, call).
 *   area = (h w) * fma(hi - lo, u, lo), u uniform in (0, 1); r one of 256 constants, the midpoints exp(log(3/4) + (k + 0.5) / 256 * log(16/9)) of the
 *   log-uniform range, k the word's top 8 bits; width = rint(sqrt(area r)), height = rint(sqrt(area / r)); accepted if 0 < width <= w and 0 < height <= h,
 *   with top = (bits * (h - height + 1)) >> 32 and left likewise.  After 10 refused tries torchvision's fallback: the whole frame if 3/4 <= w / h <= 4/3,
 *   else the centred rectangle of the nearest ratio bound.  torchvision draws log r from a continuous uniform; the 256 midpoints keep its mean and lower its
 *   variance by 1.5e-5 of itself, far below what the rounding to whole pixels does; no exp or log runs at draw time, and every float operation is one
 *   correctly rounded +, -, *, /, sqrt, fma or rint, so both functions (one inline, csrc/sample_rng.h) agree bit for bit.  torch's generator is not
 *   reproduced: the contract is the distribution plus determinism.  The result depends on (seed, call, frame, h, w, lo, hi) alone: rows lo .. hi of one
 *   draw equal a draw with first_frame = lo.  pvr_op_crop_rects refuses by name, launching nothing: a null or not 4-byte aligned rects_dev, n < 1, a
 *   negative first_frame, h or w below 1, a scale that is not finite or not 0 < lo <= hi <= 1; the host function treats such a scale as (1, 1) and writes
 *   nothing through a null pointer.
 * pvr_op_preprocess_rects: frames -> each frame's rectangle resized to crop x crop -> / 255 -> Normalize, the dense fp32 NHWC4 image.  The resize is
 *   F.interpolate(bilinear, align_corners=False) of the cropped array and round-half-even, in the rounding order of pvr_op_preprocess_windows: per frame and
 *   axis scale = (float)size / (float)crop, source index fma(scale, dst + 0.5, -0.5) clamped at 0, taps clamped to the rectangle's last row and column
 *   (not the frame's), each two-tap sum fma(w0, a, round(w1 b)) along x and then y; a crop x crop rectangle is a plain copy.  Hardened in the kernel:
 *   height is clamped to [1, h], width to [1, w], top to [0, h - height], left to [0, w - width]: no value of the array can make a lane read outside its
 *   frame or write a NaN.  color_dev == NULL: one launch, "preprocess rects", one 16-byte store per pixel.  color_dev != NULL needs gray_sums_dev and runs
 *   the launches "colour stats" and "preprocess colour" of pvr_op_preprocess_color with the rectangle as their pixel source (the same kernels,
 *   instantiated for it), with that op's checks and scratch rules; no atomics beyond its integer gray sums, two runs give the same bits.  Refused by
 *   name, launching nothing: a null frames, mean, std_, rects_dev or out_dev, a non-positive n, h, w or crop, rects_dev not 4-byte or out_dev not 16-byte
 *   aligned, more than 65535 frames, and with colour a null or misaligned gray_sums_dev, a misaligned color_dev, a crop above 256.  No Resize comes before
 *   the rectangle, so a frame smaller than the crop is legal.
 * pvr_trainer_forward_rects, rects_dev == NULL: exactly pvr_trainer_forward_augmented with null windows - the same launches, names, bits and refusals.
 *   rects_dev != NULL: "preprocess rects", or with color_dev the colour pair, stands where "preprocess" + "normalize", "preprocess windows" or the colour
 *   pair stood; everything after is unchanged, and the held forward's image is the cropped one, so conv1's weight gradient sees it.  reuse != 0 (with
 *   boundary_dev): nothing before the first trained op runs and neither array is read.  The handle keeps nothing about rectangles: a recompute pass that
 *   runs the stem again is handed the same rows again.  The descriptor's resize is not used by this path.  pvr_trainer_prefix_forward keeps the plain
 *   centre crop.  Refused by name, launching nothing: what pvr_trainer_forward_augmented refuses for boundary_dev, n, the frames and the colour
 *   arguments, and a rects_dev that is not 4-byte aligned. */
pvr_status pvr_op_crop_rects(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, int32_t h, int32_t w, float scale_lo, float scale_hi,
                             int32_t *rects_dev, void *hip_stream);
void pvr_host_crop_rects(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, int32_t h, int32_t w, float scale_lo, float scale_hi,
                         int32_t *rects_host);
pvr_status pvr_op_preprocess_rects(const uint8_t *frames_dev, int32_t n, int32_t h, int32_t w, int32_t crop, const float *mean, const float *std_,
                                   const int32_t *rects_dev, const void *color_dev, uint32_t *gray_sums_dev, float *out_dev, void *hip_stream);
pvr_status pvr_trainer_forward_rects(pvr_trainer *tr, const float *params_dev, void *bn_buffers_dev, const uint8_t *frames_dev, int32_t n, int32_t h,
                                     int32_t w, const int32_t *rects_dev, const void *color_dev, uint32_t *gray_sums_dev, float *boundary_dev,
                                     int32_t reuse, float *out_dev, int64_t out_stride, void *hip_stream);

/* Random grayscale and Gaussian blur per frame and step (the Python modes random_grayscale and gaussian_blur): the last two augmentations of MoCo v2's
 * recipe, torchvision's RandomGrayscale(p) and RandomApply([GaussianBlur(23, sigma = (lo, hi))], p) on the uint8 values of a frame's image - after the
 * window or rectangle and the colour jitter, grayscale first and blur second, before / 255 and Normalize.  A frame's parameters are two 32-bit words: float
 * sigma (0: not blurred) and int32 gray (0 or 1).  A blurred pixel is no function of one source pixel, so the image is made from a staged uint8 copy.
 * pvr_op_blur_params / pvr_host_blur_params: the parameters of frames first_frame .. first_frame + n into device / host memory (n x 2 words).  Frame f
 *   draws four words from Philox-4x32-10 with counter (f, call), as the windows do, and key (seed_lo, seed_hi ^ 0x424C5552): a stream of its own, so
 *   pvr_op_crop_windows, pvr_op_crop_rects and pvr_op_color_params keep their bits at the same (seed, call).  With u_j the uniform in the open interval
 *   (0, 1) that pvr_op_color_params makes of word j: the frame is blurred if u_0 < p_blur, with sigma = fma(hi - lo, u_1, lo) in [lo, hi], and grayed if
 *   u_2 < p_gray; p = 1 always applies and p = 0 never does.  Both functions run one inline (csrc/sample_rng.h) and agree bit for bit; the result depends on
 *   (seed, call, frame) and the four numbers alone: rows lo .. hi of one draw equal a draw with first_frame = lo.  pvr_op_blur_params refuses by name,
 *   launching nothing: a null or not 4-byte aligned blur_dev, n < 1, a negative first_frame, a probability outside [0, 1] or not finite, a sigma range
 *   that is not finite or not 0 < lo <= hi; the host function treats such a range as (1, 1) and writes nothing through a null pointer.
 * pvr_op_preprocess_staged: frames -> each frame's crop x crop uint8 pixels, 4 bytes per pixel (r, g, b, 0), into staged_dev - (n, crop, crop, 4) uint8,
 *   16-byte aligned, the caller's scratch as gray_sums_dev is.  The pixel source is the window (windows_dev, as pvr_op_preprocess_windows reads it, with
 *   resize) or the rectangle (rects_dev, as pvr_op_preprocess_rects reads it; resize is not used), exactly one of them.  color_dev != NULL needs
 *   gray_sums_dev and runs the launch "colour stats" of pvr_op_preprocess_color as it is, then the frame's colour ops on every pixel.  Then ONE launch,
 *   "stage image".  It runs the device inlines of the un-staged kernels, so the staged bytes are exactly the uint8 values those kernels normalise.
 *   Refused by name, launching nothing: a null frames_dev or staged_dev, both or neither pixel source, what the source's own op refuses for n, h, w,
 *   crop and the alignment of its array, staged_dev not 16-byte aligned, more than 65535 frames, and with colour a null or misaligned gray_sums_dev, a
 *   misaligned color_dev, a crop above 256.
 * pvr_op_blur_normalize: the staged pixels -> per frame grayscale if flagged (trunc(((0.2989 r) + (0.587 g)) + (0.114 b)) on all three channels:
 *   rgb_to_grayscale(num_output_channels = 3) on uint8), blur if sigma > 0, (v / 255 - mean) / std into the dense fp32 NHWC4 image: one launch, "blur
 *   normalize".  The blur is torchvision's gaussian_blur on a uint8 tensor with kernel size 23 (fixed; PIL's radius semantics are not offered): 1-D weights
 *   pdf_i = exp(-0.5 (i / sigma)^2), i = -11 .. 11, over their sum, the 2-D kernel their outer product, reflect padding of 11, the sum in fp32 with no
 *   rounding between the two axes, then round-half-even to uint8.  The kernel sums the two axes one after the other (a separable filter in LDS:
 *   csrc/preprocess.hip), torchvision all 529 products at once: the fp32 sums differ by rounding alone, so the uint8 result equals the exactly rounded
 *   one except where the exact sum lies within 1.9e-3 of a .5 tie (tests/gaussian_blur_refs.py derives the bound), and is never more than one step
 *   off.  Hardened in the kernel: a NaN or non-positive sigma means no blur, sigma is clamped to at most 16, tap 0's pdf is 1 by definition (a tiny sigma
 *   is the identity, never 0 / 0), a non-zero gray word counts as 1, every read is reflected and clamped into the frame: no value of blur_dev can produce
 *   a NaN image or a read outside the frame.  Plain vector loads and stores, no atomics: two runs give the same bits.  A frame with sigma 0 and gray 0
 *   gets the bits of the un-staged kernels.  Refused by name, launching nothing: a null staged_dev, mean, std_, blur_dev or out_dev, staged_dev or out_dev
 *   not 16-byte or blur_dev not 4-byte aligned, n < 1, crop < 12 (a reflect padding of 11 needs 12 pixels), crop > 256, more than 65535 frames.
 * pvr_trainer_forward_staged: pvr_trainer_forward_rects plus windows_dev, blur_dev and staged_dev.  blur_dev == NULL: exactly pvr_trainer_forward_rects
 *   (with rects_dev) or pvr_trainer_forward_augmented (without) - the same launches, names, bits and refusals.  blur_dev != NULL needs staged_dev and
 *   exactly one of windows_dev and rects_dev (the centre window for every frame where no random crop is wanted, as the colour jitter does): "stage image"
 *   (with color_dev "colour stats" before it) and "blur normalize" stand where the image launches stood; everything after is unchanged, and the held
 *   forward's image is the augmented one, so conv1's weight gradient sees it.  reuse != 0 (with boundary_dev): nothing before the first trained op runs
 *   and no array is read.  The handle keeps nothing about the parameters: a recompute pass that runs the stem again is handed the same rows again.
 *   pvr_trainer_prefix_forward keeps the plain centre crop.  Refused by name, launching nothing: what pvr_trainer_forward_rects refuses, both or neither
 *   pixel source, a misaligned windows_dev or blur_dev, a null or misaligned staged_dev, a crop outside 12 .. 256. */
pvr_status pvr_op_blur_params(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, float p_blur, float sigma_lo, float sigma_hi, float p_gray,
                              void *blur_dev, void *hip_stream);
void pvr_host_blur_params(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, float p_blur, float sigma_lo, float sigma_hi, float p_gray,
                          void *blur_host);
pvr_status pvr_op_preprocess_staged(const uint8_t *frames_dev, int32_t n, int32_t h, int32_t w, int32_t resize, int32_t crop, const int32_t *windows_dev,
                                    const int32_t *rects_dev, const void *color_dev, uint32_t *gray_sums_dev, void *staged_dev, void *hip_stream);
pvr_status pvr_op_blur_normalize(const void *staged_dev, int32_t n, int32_t crop, const float *mean, const float *std_, const void *blur_dev,
                                 float *out_dev, void *hip_stream);
pvr_status pvr_trainer_forward_staged(pvr_trainer *tr, const float *params_dev, void *bn_buffers_dev, const uint8_t *frames_dev, int32_t n, int32_t h,
                                      int32_t w, const int32_t *windows_dev, const int32_t *rects_dev, const void *color_dev, uint32_t *gray_sums_dev,
                                      const void *blur_dev, void *staged_dev, float *boundary_dev, int32_t reuse, float *out_dev, int64_t out_stride,
                                      void *hip_stream);

/* per-launch timing (scripts/train_step_times.py): on != 0 brackets every launch of the following forwards / backwards with
 * events (the calls then synchronise); pvr_trainer_launch_time reads launch `index` of the last forward + backward: its name,
 * milliseconds and algorithmic FLOPs (0 for byte kernels); returns the name's length, 0 past the end */
pvr_status pvr_trainer_debug_set_timing(pvr_trainer *tr, int32_t on);
int32_t pvr_trainer_launch_time(const pvr_trainer *tr, int32_t index, char *name, int32_t cap, float *ms, double *flops);

/* ---------------------------------------------------------------------------------------------
 * The trainer's kernels one at a time (unit-parity entry points).  All tensors fp32 NHWC on the device; an unsupported shape
 * returns a status with a message and launches nothing.  scratch_dev: fp32 device scratch of at least the matching
 * *_scratch_floats() values.
 * ------------------------------------------------------------------------------------------- */
/* BatchNorm2d, training mode, over `rows` = n*h*w rows of c channels (c % 4 == 0, rows >= 2): two-pass batch mean and biased
 * variance; y = (z - mean) * rstd * gamma + beta [+ residual] [ReLU]; mean_out / rstd_out (c floats each) are what the backward
 * needs.  running_mean / running_var / num_batches_tracked (int64) are updated when given (all three or none). */
int64_t pvr_op_bn_scratch_floats(int64_t rows, int32_t c);
pvr_status pvr_op_bn_train_forward(const float *z_dev, const float *residual_dev, const float *gamma_dev, const float *beta_dev, float *running_mean_dev,
                                   float *running_var_dev, int64_t *num_batches_tracked_dev, float *y_dev, float *mean_out_dev, float *rstd_out_dev,
                                   int64_t rows, int32_t c, int32_t relu, float *scratch_dev, int64_t scratch_floats, void *hip_stream);
/* its backward: g = dy where (relu == 0 or y > 0) else 0; dgamma = sum g * xhat, dbeta = sum g; dz = gamma * rstd * (g - dbeta / rows - xhat * dgamma / rows);
 * dres (optional) = g, added to what it holds when dres_accumulate != 0 */
pvr_status pvr_op_bn_train_backward(const float *z_dev, const float *y_dev, const float *dy_dev, const float *gamma_dev, const float *mean_dev,
                                    const float *rstd_dev, float *dz_dev, float *dres_dev, int32_t dres_accumulate, float *dgamma_dev, float *dbeta_dev,
                                    int64_t rows, int32_t c, int32_t relu, float *scratch_dev, int64_t scratch_floats, void *hip_stream);
/* BatchNorm2d on its RUNNING statistics (frozen BatchNorm), rows >= 1, c % 4 == 0: y = (z - running_mean) * rstd * gamma + beta [+ residual] [ReLU] with
 * rstd = 1 / sqrt(running_var + 1e-5), one pass over z, no scratch; mean_out / rstd_out (c floats each) receive running_mean and rstd for the backward.
 * running_mean / running_var are read only. */
pvr_status pvr_op_bn_frozen_forward(const float *z_dev, const float *residual_dev, const float *gamma_dev, const float *beta_dev,
                                    const float *running_mean_dev, const float *running_var_dev, float *y_dev, float *mean_out_dev, float *rstd_out_dev,
                                    int64_t rows, int32_t c, int32_t relu, void *hip_stream);
/* A frozen prefix op (pvr_trainer_set_train_from) as ONE convolution launch behind the weight pack: y (n,ho,wo,cout) = (conv(x (n,h,w,cin), w torch's
 * (cout,cin,k,k)) - running_mean) * rstd * gamma + beta [+ residual] [ReLU], rstd = 1 / sqrtf(running_var + 1e-5) evaluated per channel in the kernel.
 * The convolution is pvr_op_conv2d_f32's single fp32 fma chain over K = k*k*cin in the same order, the epilogue pvr_op_bn_frozen_forward's expression
 * per element; no pre-BN tensor and no mean / rstd are written.  The scratch holds the packed weights.  cin % 32 == 0, cout % 4 == 0, k 1 .. 3,
 * stride 1 or 2, pad < k, every operand below 2 GiB; anything else is refused by name and launches nothing.  Two runs give the same bits. */
int64_t pvr_op_conv_bn_frozen_forward_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad);
pvr_status pvr_op_conv_bn_frozen_forward(const float *x_dev, const float *w_dev, const float *gamma_dev, const float *beta_dev, const float *running_mean_dev,
                                         const float *running_var_dev, const float *residual_dev, float *y_dev, int32_t n, int32_t h, int32_t w, int32_t cin,
                                         int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t relu, float *scratch_dev, int64_t scratch_floats,
                                         void *hip_stream);
/* its backward (arguments as pvr_op_bn_train_backward, scratch of pvr_op_bn_scratch_floats): g = dy where (relu == 0 or y > 0) else 0;
 * dbeta = sum g; dgamma = sum g * xhat, xhat = (z - mean) * rstd; dz = gamma * rstd * g (the statistics are constants: no mean terms);
 * dres (optional) = g, added to what it holds when dres_accumulate != 0.  One kernel streams z, y, dy -> dz, dres and writes per-block partial
 * sums, a second sums them in double in block order: no float atomics, two runs give the same bits. */
pvr_status pvr_op_bn_frozen_backward(const float *z_dev, const float *y_dev, const float *dy_dev, const float *gamma_dev, const float *mean_dev,
                                     const float *rstd_dev, float *dz_dev, float *dres_dev, int32_t dres_accumulate, float *dgamma_dev, float *dbeta_dev,
                                     int64_t rows, int32_t c, int32_t relu, float *scratch_dev, int64_t scratch_floats, void *hip_stream);
/* Weight gradient of a k x k convolution (k 1 or 3, stride 1 or 2, cin % 32 == 0, cout % 4 == 0) on the f32-input MFMA:
 * dw[co][ci][kh][kw] = sum over (n, y, x) of dz[n,y,x,co] * x[n, y*stride + kh - pad, x*stride + kw - pad, ci]; x (n,h,w,cin),
 * dz (n,ho,wo,cout), dw in torch's (cout, cin, k, k) layout.  The pixel range is split over workgroups and the partials are summed in a fixed order. */
int64_t pvr_op_conv_wgrad_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad);
pvr_status pvr_op_conv_wgrad(const float *x_dev, const float *dz_dev, float *dw_dev, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k,
                             int32_t stride, int32_t pad, float *scratch_dev, int64_t scratch_floats, void *hip_stream);
/* Data gradient of the same convolution: dx (n,h,w,cin) [+= when accumulate != 0] conv(dz written to the even pixels of a zeroed (h, w) grid when stride == 2,
 * rot180(W) transposed, stride 1, pad k - 1 - pad) through pvr_op_conv2d_f32's kernel.  w: torch's (cout, cin, k, k).  (k, pad) = (3, 1) or (1, 0),
 * cout % 32 == 0, cin % 4 == 0; stride 2 needs even h and w (an odd size is refused). */
int64_t pvr_op_conv_dgrad_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad);
pvr_status pvr_op_conv_dgrad(const float *dz_dev, const float *w_dev, float *dx_dev, int32_t accumulate, int32_t n, int32_t h, int32_t w, int32_t cin,
                             int32_t cout, int32_t k, int32_t stride, int32_t pad, float *scratch_dev, int64_t scratch_floats, void *hip_stream);
/* Weight gradient of conv1 (7x7 / 2, pad 3): img the normalised NHWC4 image (n,S,S,4), dz (n,S/2,S/2,64), dw torch's (64,3,7,7).  S even. */
int64_t pvr_op_stem_wgrad_scratch_floats(int32_t n, int32_t S);
pvr_status pvr_op_stem_wgrad(const float *img_dev, const float *dz_dev, float *dw_dev, int32_t n, int32_t S, float *scratch_dev, int64_t scratch_floats,
                             void *hip_stream);
/* s = 2^(14 - floor(log2 max|x|)) over `count` floats, written to the device float scale_dev: the scaled maximum lies in [2^14, 2^15), inside f16's
 * normal range.  An all-zero (or empty) tensor and a non-finite maximum give 1; the exponent is clamped to [-126, 126] so that s and 1 / s are normal
 * fp32 numbers.  The maximum is an integer max over the bit patterns of |x| (order-independent, so deterministic); no host synchronisation - the
 * consumers read the scale from device memory. */
pvr_status pvr_op_absmax_scale(const float *x_dev, int64_t count, float *scale_dev, void *hip_stream);
/* the same rule for one or two tensors in ONE launch (the trainer's form: dz and, on its first use in a backward, the saved activation).  x1_dev and
 * scale1_dev may both be null.  aux_dev: four uint32 of device memory that are zero on entry - the caller zeroes them once - and zero again when the
 * launch has finished (per tensor a running maximum and a count of finished blocks; the block that finishes last writes the scale). */
pvr_status pvr_op_absmax_scale_pair(const float *x0_dev, int64_t count0, float *scale0_dev, const float *x1_dev, int64_t count1, float *scale1_dev,
                                    uint32_t *aux_dev, void *hip_stream);
/* pvr_op_conv_wgrad (same shapes, layouts and refusals) as an exact-split product on the f16 matrix pipe: x and dz are multiplied by *x_scale_dev and
 * *dz_scale_dev (powers of two, from pvr_op_absmax_scale), split in registers into hi = f16(a'), lo = f16((a' - hi) * 2048), and every fragment pair
 * takes three v_mfma_f32_16x16x32_f16 (hi*hi; the two cross terms into a second accumulator scaled by 2^-11 once).  The partials of the pixel ranges
 * are summed in split order in double; that reduction undoes the two scales (exact) and writes torch's (cout, cin, k, k).  Two runs give the same bits.
 * |error| <= (L + 20) 2^-24 sum|dz||x| + 2^-27 (max|x| sum|dz| + max|dz| sum|x|) per element, L the pixels of the sum. */
int64_t pvr_op_conv_wgrad_split16_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad);
pvr_status pvr_op_conv_wgrad_split16(const float *x_dev, const float *dz_dev, float *dw_dev, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                     int32_t k, int32_t stride, int32_t pad, const float *x_scale_dev, const float *dz_scale_dev, float *scratch_dev,
                                     int64_t scratch_floats, void *hip_stream);
/* pvr_op_stem_wgrad (conv1, 7x7 / 2, pad 3; img (n,S,S,4), dz (n,S/2,S/2,64), dw (64,3,7,7), S even) as the same split product: 64 couts x 196
 * (tap, channel) columns, gathered from the unpadded image with border masks, reduced over the n (S/2)^2 output pixels. */
int64_t pvr_op_stem_wgrad_split16_scratch_floats(int32_t n, int32_t S);
pvr_status pvr_op_stem_wgrad_split16(const float *img_dev, const float *dz_dev, float *dw_dev, int32_t n, int32_t S, const float *img_scale_dev,
                                     const float *dz_scale_dev, float *scratch_dev, int64_t scratch_floats, void *hip_stream);
/* z (n,ho,wo,cout) = conv(x (n,h,w,cin), w torch's (cout,cin,k,k)) without bias, as an exact-split product on the f16 matrix pipe: x times *x_scale_dev
 * and w times *w_scale_dev (powers of two from pvr_op_absmax_scale, read on the device), each scaled value split into hi = f16(a'), lo = f16((a' - hi)
 * * 2048); a pack launch writes the split weights to the scratch, the convolution takes three v_mfma_f32_16x16x32_f16 per fragment pair (hi*hi; the two
 * cross terms into a second accumulator scaled by 2^-11 once) and its epilogue multiplies by 1 / s_x and 1 / s_w (exact).  k 1..3, stride 1 or 2,
 * pad < k, cin % 32 == 0, cout % 4 == 0; every operand below 2 GiB.  Two runs give the same bits.
 * |error| <= (K + 20) 2^-24 sum|x||w| + 2^-27 (max|x| sum|w| + max|w| sum|x|) per element, K = k*k*cin the products of the sum. */
int64_t pvr_op_conv_fwd_split16_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad);
pvr_status pvr_op_conv_fwd_split16(const float *x_dev, const float *w_dev, float *z_dev, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k,
                                   int32_t stride, int32_t pad, const float *x_scale_dev, const float *w_scale_dev, float *scratch_dev, int64_t scratch_floats,
                                   void *hip_stream);
/* pvr_op_conv_bn_frozen_forward on the split product: the arguments of that entry point plus the two scales, the shapes and refusals of
 * pvr_op_conv_fwd_split16.  The pack launch of pvr_op_conv_fwd_split16 followed by ONE launch whose K loop and scale undoing are that convolution's and
 * whose epilogue is pvr_op_bn_frozen_forward's expression in the same order of roundings: y has the bits of pvr_op_conv_fwd_split16 followed by
 * pvr_op_bn_frozen_forward on the same inputs and scales.  No pre-BN tensor, mean or rstd is written; the running statistics are read only. */
int64_t pvr_op_conv_bn_frozen_forward_split16_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride,
                                                             int32_t pad);
pvr_status pvr_op_conv_bn_frozen_forward_split16(const float *x_dev, const float *w_dev, const float *gamma_dev, const float *beta_dev,
                                                 const float *running_mean_dev, const float *running_var_dev, const float *residual_dev, float *y_dev, int32_t n,
                                                 int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t relu,
                                                 const float *x_scale_dev, const float *w_scale_dev, float *scratch_dev, int64_t scratch_floats,
                                                 void *hip_stream);
/* pvr_op_conv_dgrad (same shapes, layouts and refusals) as the same split product: the pack launch writes the rotated, transposed split weights, a
 * stride-2 convolution's dz goes to the even pixels of the zeroed grid (its scale is dz's: zeros do not move a maximum), and the epilogue adds what
 * dx holds when accumulate != 0 (one fp32 addition; the bound gains 2^-24 (|previous| + |result|)).  K = k*k*cout. */
int64_t pvr_op_conv_dgrad_split16_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad);
pvr_status pvr_op_conv_dgrad_split16(const float *dz_dev, const float *w_dev, float *dx_dev, int32_t accumulate, int32_t n, int32_t h, int32_t w, int32_t cin,
                                     int32_t cout, int32_t k, int32_t stride, int32_t pad, const float *dz_scale_dev, const float *w_scale_dev,
                                     float *scratch_dev, int64_t scratch_floats, void *hip_stream);
/* MaxPool2d(3, 2, 1) backward as a gather: x (n,h,w,c) the pool's input, dy (n,ho,wo,c), dx (n,h,w,c) fully written; a tie goes to the first maximum of a
 * window in scan order (torch's rule) */
pvr_status pvr_op_maxpool_backward(const float *x_dev, const float *dy_dev, float *dx_dev, int32_t n, int32_t h, int32_t w, int32_t c, void *hip_stream);
/* AdaptiveAvgPool2d(1) backward: dx[(i*hw + p)*c + ch] = dout[i*dout_stride + ch] / hw */
pvr_status pvr_op_avgpool_backward(const float *dout_dev, int64_t dout_stride, float *dx_dev, int32_t n, int32_t hw, int32_t c, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* PVR_TRAIN_H */
