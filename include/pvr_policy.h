/*
 * pvr_policy.h — C-ABI of the behavioural-cloning policy path in libpvr_hip.so (fp32).
 *
 * Replaces, for the reference's hot path:
 *   src/models.py:57-89      PolicyNet.forward  ([BatchNorm1d] -> FC+ReLU -> FC+ReLU -> 2-layer LSTM stepped
 *                            one timestep at a time with state *= (1-done) -> policy/baseline heads -> argmax)
 *   main_bc_2.py:206-227     one training iteration: nll_loss(log_softmax) mean, backward (BPTT), sum of squared
 *                            grad norms, clip_grad_norm_(max_norm), RMSprop(momentum=0) with the LambdaLR factor
 *                            already applied by the caller (lr argument)
 * Parameters live in ONE flat fp32 device buffer owned by the caller (PyTorch parameters are views of it);
 * pvr_policy_param_offset gives each tensor's offset under its reference state_dict name
 * ("fc.1.weight", "core.weight_hh_l0", ...).  Trainable tensors come first; the baseline head (which
 * receives no gradient from the BC loss, so torch leaves its .grad None) is last and is excluded from
 * the grad norm and the update, exactly as in the reference.
 */
#ifndef PVR_POLICY_H
#define PVR_POLICY_H

#include "pvr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pvr_policy pvr_policy;

typedef struct pvr_policy_desc {
    int32_t obs_size;      /* observation_shape[0] (models.py:22) */
    int32_t hidden;        /* 1024 in the reference; multiple of 1024 */
    int32_t num_actions;   /* <= 16 */
    int32_t batch_norm;    /* BatchNorm1d in front of the MLP (models.py:30-34) */
    int32_t max_t;         /* unroll_length the workspace is sized for */
    int32_t max_b;         /* batch_size the workspace is sized for (<= 64) */
    int32_t conv_frames;   /* 0: vector observations (PolicyNet).  n > 0: PolicyNetWithConv (models.py:96-197) on raw uint8
                              (T,B,64,64,3n) observations; obs_size must be 128*n and `obs` arguments are uint8 */
} pvr_policy_desc;

pvr_status pvr_policy_create(const pvr_policy_desc *desc, pvr_policy **out);
/* The same handle on the HOST (CPU) backend - BASELINE configs[0] runs main_bc_2.py's policy without a GPU, and the reference's model
 * lives wherever flags.device says (main_bc_2.py:64-66).  No HIP call is made; params / square_avg / BatchNorm buffers / obs / done /
 * actions / outputs of pvr_policy_forward and pvr_policy_step are HOST pointers, hip_stream is ignored, and the arithmetic is plain fp32
 * C++ on this process's threads (PVR_HOST_THREADS).  Vector observations only (conv_frames must be 0); the split entry points
 * (backward / apply / backward_dlogits / data parallel) belong to the HIP plan and are refused. */
pvr_status pvr_policy_create_host(const pvr_policy_desc *desc, pvr_policy **out);
void pvr_policy_destroy(pvr_policy *pol);

/* number of fp32 elements of the flat parameter buffer, and of its trainable prefix */
int64_t pvr_policy_param_count(const pvr_policy *pol);
int64_t pvr_policy_trainable_count(const pvr_policy *pol);
/* offset (elements) and size of a tensor by reference state_dict name; returns -1 if unknown */
int64_t pvr_policy_param_offset(const pvr_policy *pol, const char *name, int64_t *numel);

/* BatchNorm1d buffers (device): running_mean, running_var (fp32, obs_size) and num_batches_tracked (int64[1]);
 * ignored when batch_norm == 0 */
typedef struct pvr_policy_bn {
    float *running_mean;
    float *running_var;
    int64_t *num_batches_tracked;
} pvr_policy_bn;

/* Data-parallel finetune (BASELINE config 4; the reference's main_bc_finetune.py:167-208 is single-GPU and src/models.py:132-136
 * is a plain BatchNorm1d).  The caller hands the library ONE collective as a C function pointer:
 *     fn(buf, count, hip_stream, user) = in-place SUM all-reduce over the ranks of `count` fp32 values at device address `buf`,
 *     enqueued on hip_stream (RCCL over xGMI: ncclAllReduce, or torch.distributed.all_reduce under backend "nccl"); returns 0 on
 *     success, non-zero makes the calling entry point fail with PVR_ERR_COMM.
 * With world_size > 1 installed, pvr_policy_backward / pvr_policy_step on every rank
 *   - all-reduce the gradient in four buckets, in the order backward finalises them (LSTM layer 1 + policy head, LSTM layer 0,
 *     the two fc layers, conv stack + BatchNorm affine), each on a library-owned communication stream that waits only for the
 *     event recorded after the bucket's last kernel, so the transfers overlap the rest of the backward pass; the buckets (and
 *     the loss) are divided by world_size there and the compute stream re-joins before the entry point returns: `grads` then
 *     holds the gradient of the GLOBAL batch mean and stats_out[0] the global loss;
 *   - with sync_bn != 0, use BatchNorm statistics of the global batch (world_size x T x B rows, equal rows per rank): per-rank
 *     column sums are all-reduced on the compute stream between the statistic kernels (mean, centred second moment, and - for
 *     PolicyNetWithConv - the two backward sums), so N ranks x B/N sequences equal one rank x B.
 * world_size <= 1 or fn == NULL restores single-rank behaviour. */
typedef int32_t (*pvr_allreduce_fn)(void *buf_dev, int64_t count, void *hip_stream, void *user);
#define PVR_ERR_COMM 5
#define PVR_ERR_TIMEOUT 6
pvr_status pvr_policy_set_data_parallel(pvr_policy *pol, int32_t world_size, int32_t sync_bn, pvr_allreduce_fn fn, void *user);

/* Health of the handle's persistent launches.  The forward recurrence (models.py:66-73) may run as ONE launch per layer whose
 * blocks hand h_t to each other inside the kernel; it is only chosen when the whole grid fits the GPU at once (occupancy x CU count,
 * checked at create), its waits are bounded, and a wait that runs out stores into a pinned status word (and poisons that call's
 * outputs with NaN).  pvr_policy_status returns PVR_ERR_TIMEOUT once for such an event (message via pvr_last_error) and the handle
 * falls back to per-step launches; pvr_policy_forward / _backward / _backward_dlogits / _step perform the same check on entry, so a
 * time-out never goes unnoticed.  It does not synchronise: call it after the stream has been synchronised to learn about the
 * launches just enqueued.  (The reference has no counterpart: nn.LSTM cannot time out.)
 * pvr_policy_recurrence_mode: 0 per-step launches, 1 / 2 persistent (counter / data-as-flag hand-off) - what the next forward will use. */
pvr_status pvr_policy_status(pvr_policy *pol);
int32_t pvr_policy_recurrence_mode(const pvr_policy *pol);
/* test hook: block `block` (>= 0) of every following persistent launch exits at once, so its peers' waits run out and the failure
 * path above can be exercised on a healthy GPU (tests/test_gpu_policy.py); -1 restores normal launches */
pvr_status pvr_policy_debug_drop_block(pvr_policy *pol, int32_t block);

/* PolicyNet.forward (models.py:57-89).  obs (T,B,obs_size) fp32 (uint8 (T,B,64,64,3n) when conv_frames = n > 0), done (T,B) uint8, h0/c0 (2,B,hidden) fp32 are
 * device inputs; logits (T,B,A), baseline (T,B), action (T,B) int64 = argmax (eval branch, :82; a sample in training mode after pvr_policy_set_action_sampling), h_out/c_out
 * (2,B,hidden) are device outputs.  training != 0 uses batch statistics and updates the BN buffers (:31-34). */
/* Training-mode action of PolicyNet.forward (models.py:78-80: torch.multinomial(F.softmax(policy_logits, dim=1), num_samples=1)).  With
 * on != 0 every following training-mode pvr_policy_forward writes ONE SAMPLE of softmax(logits) per row into `action` instead of the
 * argmax, drawn inside the heads kernel (Gumbel-max over a counter-based Philox-4x32-10 stream keyed by `seed` and counted by call and
 * row: reproducible for a seed, independent of the launch geometry; torch's own generator stream is not reproduced - the contract is the
 * distribution).  Calling it again restarts the stream.  Eval-mode forwards and pvr_policy_step are unaffected.  Default off. */
pvr_status pvr_policy_set_action_sampling(pvr_policy *pol, int32_t on, uint64_t seed);
/* Position of that stream = the number of sampling forwards since pvr_policy_set_action_sampling; a caller that replaces a handle (larger
 * T / B, another device) reads it from the old handle and sets it on the new one, so the noise stream continues instead of replaying
 * (the reference's torch.multinomial consumes the global generator, which no module re-arms: src/models.py:78-80). */
uint64_t pvr_policy_action_sampling_call(const pvr_policy *pol);
pvr_status pvr_policy_set_action_sampling_call(pvr_policy *pol, uint64_t call);
pvr_status pvr_policy_forward(pvr_policy *pol, const float *params, const pvr_policy_bn *bn, const void *obs,
                              const uint8_t *done, const float *h0, const float *c0, int32_t T, int32_t B,
                              int32_t training, float *logits, float *baseline, int64_t *action, float *h_out,
                              float *c_out, void *hip_stream);

/* One iteration of main_bc_2.py:206-227 from a zero initial state: forward (training), loss, backward,
 * grad-norm, clip, RMSprop.  params / square_avg: flat device buffers (updated in place).  actions (T,B) int64.
 * lr = learning_rate * LambdaLR factor for this update.  stats_out (device, 2 floats): loss, grad norm (pre-clip).
 * logits_out (optional, may be NULL): (T,B,A) training-mode logits. */
pvr_status pvr_policy_step(pvr_policy *pol, float *params, float *square_avg, const pvr_policy_bn *bn,
                           const void *obs, const uint8_t *done, const int64_t *actions, int32_t T, int32_t B,
                           float lr, float alpha, float eps, float max_grad_norm, float *stats_out,
                           float *logits_out, void *hip_stream);

/* The same iteration in two halves (data-parallel training, autograd bridge).  pvr_policy_backward leaves the UNCLIPPED
 * gradient of the mean loss in grads (device, trainable_count floats, caller-owned) and the loss in stats_out[0] - the local
 * batch's, or the global batch's when pvr_policy_set_data_parallel is installed; pvr_policy_apply computes the norm of whatever
 * grads holds, clips and applies RMSprop; stats_out[1] = that norm. */
pvr_status pvr_policy_backward(pvr_policy *pol, const float *params, const pvr_policy_bn *bn, const void *obs,
                               const uint8_t *done, const int64_t *actions, int32_t T, int32_t B, float *grads,
                               float *stats_out, float *logits_out, void *hip_stream);
pvr_status pvr_policy_apply(pvr_policy *pol, float *params, float *square_avg, const float *grads, float lr,
                            float alpha, float eps, float max_grad_norm, float *stats_out, void *hip_stream);

/* Autograd bridge: the backward half for a caller that computes the loss itself (the reference's own lines, main_bc_2.py:211-220:
 * F.nll_loss(F.log_softmax(logits)) ... loss.backward()).  Call after a training-mode pvr_policy_forward of the same (obs, T, B):
 * dlogits (device, (T,B,A) contiguous) is d(loss)/d(policy_logits); leaves d(loss)/d(params) in grads (trainable_count floats) -
 * all-reduced over the ranks when pvr_policy_set_data_parallel is installed.  The baseline head receives no gradient (the BC loss
 * does not read it; torch leaves its .grad None too).  One backward per forward. */
pvr_status pvr_policy_backward_dlogits(pvr_policy *pol, const float *params, const void *obs, const float *dlogits, int32_t T,
                                       int32_t B, float *grads, void *hip_stream);

/* End-to-end BC (the observations are the output of a trainable encoder, pvr_train.h): the two backward entry points above with one more output.
 * dobs (device, (T,B,obs_size) contiguous fp32, 16-byte aligned, caller-owned) is fully overwritten with d(loss)/d(obs) - of the mean NLL for
 * pvr_policy_backward_dobs, of whatever dlogits encodes for pvr_policy_backward_dlogits_dobs:
 *     without BatchNorm   dobs = dz1 W_fc1
 *     with BatchNorm1d    dobs = gamma invstd (da0 - sum(da0) / N - xhat sum(da0 xhat) / N),  da0 = dz1 W_fc1, N = T B  (torch's training-mode rule)
 * dobs == NULL is the entry point above: the same launches.  Asking for dobs does not change a bit of `grads`: its launches follow the ones that
 * finish the parameter gradient.  PVR_ERR_INVALID (message names the cause) for conv_frames > 0 (uint8 observations have no gradient), a host
 * handle, and an installed data-parallel collective (encoder training is single-GPU). */
pvr_status pvr_policy_backward_dobs(pvr_policy *pol, const float *params, const pvr_policy_bn *bn, const void *obs, const uint8_t *done,
                                    const int64_t *actions, int32_t T, int32_t B, float *grads, float *stats_out, float *logits_out,
                                    float *dobs, void *hip_stream);
pvr_status pvr_policy_backward_dlogits_dobs(pvr_policy *pol, const float *params, const void *obs, const float *dlogits, int32_t T,
                                            int32_t B, float *grads, float *dobs, void *hip_stream);

/* clip_grad_norm_ + RMSprop(momentum 0) over SEVERAL flat buffers with ONE norm (end-to-end BC: the policy's trainable prefix and the encoder's
 * parameters; the reference clips over all parameters together).  Semantics of pvr_policy_apply: coef = min(1, max_norm / (norm + 1e-6)),
 * v = alpha v + (1 - alpha) g^2, p -= lr g / (sqrt(v) + eps) with g the clipped gradient.  n_groups <= 8, counts[i] % 4 == 0, every buffer
 * 16-byte aligned; the arrays of pointers and counts are host memory, the buffers device memory.  The norm is summed in a fixed order (256
 * partials per group, then in group order; no float atomics): two runs give the same bits.  stats_out (device, 1 float, may be NULL) = the
 * pre-clip norm over all groups.  No handle; calls on one stream are ordered. */
pvr_status pvr_joint_apply_rmsprop(int32_t n_groups, float *const *params, float *const *square_avg, const float *const *grads,
                                   const int64_t *counts, float lr, float alpha, float eps, float max_grad_norm, float *stats_out,
                                   void *hip_stream);

/* Other update rules on the same flat buffers (grad norm + clip as in pvr_policy_apply; stats_out[1] = pre-clip norm):
 * torch.optim.RMSprop with momentum != 0 (src/arguments.py:63 exposes --momentum; the reference default 0 is pvr_policy_apply) and
 * torch.optim.Adam(betas, eps; amsgrad off, no weight decay) - an extension, BASELINE.json's north_star names Adam.  step = 1, 2, ...
 * is the update count (bias correction). */
pvr_status pvr_policy_apply_momentum(pvr_policy *pol, float *params, float *square_avg, float *momentum_buf, const float *grads,
                                     float lr, float alpha, float eps, float momentum, float max_grad_norm, float *stats_out,
                                     void *hip_stream);
pvr_status pvr_policy_apply_adam(pvr_policy *pol, float *params, float *exp_avg, float *exp_avg_sq, const float *grads, float lr,
                                 float beta1, float beta2, float eps, int64_t step, float max_grad_norm, float *stats_out,
                                 void *hip_stream);

/* BC batch assembly on the device: replaces the host gather of main_bc_2.py:186-204 (identical in main_bc_1.py:193-211 and
 * main_bc_finetune.py:173-188).  The dataset stays resident in HBM: obs_dev (n_samples rows of row_bytes bytes: fp32 embeddings, or
 * raw uint8 frames for the finetune model), action_dev (int64), done_dev (uint8).  For the B start indices of
 * sample_with_minimum_distance (starts_dev, int64) row (t, b) of every output is dataset row (starts[b] + t) mod n_samples, i.e.
 * out_obs is the (T, B, ...) batch np.stack(..., axis=1) builds.  action / done may both be NULL. */
pvr_status pvr_bc_gather(const void *obs_dev, const int64_t *action_dev, const uint8_t *done_dev, int64_t n_samples,
                         int64_t row_bytes, const int64_t *starts_dev, int32_t T, int32_t B, void *out_obs,
                         int64_t *out_action, uint8_t *out_done, void *hip_stream);

/* parity/debug: copy the flat gradient of the last pvr_policy_step (pre-clip) to grads_out (device, trainable_count) */
pvr_status pvr_policy_last_grads(pvr_policy *pol, float *grads_out, void *hip_stream);

/* parity/debug: d(loss)/d(policy_logits) of the last backward of T x B rows, (T,B,A) contiguous, as the backward read it - the loss kernel's
 * (softmax - onehot) / (T B) after pvr_policy_backward / _backward_dobs / _step, the caller's own after pvr_policy_backward_dlogits[_dobs].  Handing
 * it to pvr_policy_backward_dlogits_dobs after a forward of the same inputs reproduces that backward bit for bit (tests/test_gpu_e2e_bc.py: torch's
 * log_softmax rounds differently from the loss kernel, so the two forms of an iteration agree in every bit only on the same upstream gradient). */
pvr_status pvr_policy_last_dlogits(pvr_policy *pol, float *dlogits_out, int32_t T, int32_t B, void *hip_stream);

/* fp32-in / fp32-out GEMM as the policy runs it: C[M,N] = op(A) op(B)^T-style contraction over K.
 * a_km != 0: A stored [K][M] else [M][K];  b_kn != 0: B stored [K][N] else [N][K].  Optional bias[N], relu.
 * (unit-parity entry point; the arithmetic is the one pvr_debug_set_gemm_mode selects) */
pvr_status pvr_op_gemm_f32(const float *A, const float *B, const float *bias, float *C, int32_t M, int32_t N,
                           int32_t K, int32_t a_km, int32_t b_kn, int32_t relu, void *hip_stream);
/* pvr_op_gemm_f32 with the backward pass's ReLU mask: C[m][n] = 0 where mask[m][n] <= 0 (mask [M][N] fp32, may be NULL), applied after bias and relu -
 * in the GEMM kernel, or in the slice sum when the shape takes split-K */
pvr_status pvr_op_gemm_f32_masked(const float *A, const float *B, const float *bias, const float *mask, float *C, int32_t M, int32_t N,
                                  int32_t K, int32_t a_km, int32_t b_kn, int32_t relu, void *hip_stream);

/* Unit entry points of the policy's kernels (tests/test_gpu_policy_kernels.py holds each to a float64 reference).  No handle, no state: device pointers
 * and a stream; each enqueues exactly the launches pvr_policy_forward / _backward enqueue for that operation, through the same launch code.  Buffers
 * read as float4s must be 16-byte aligned (refused otherwise).
 * `form` of a reduction over R rows: -1 as the plan chooses (two-stage from R >= 512 when the column count is a multiple of 4), 0 one launch,
 * 1 two-stage (row groups of 64, then a fixed-order sum of the group partials).  pvr_debug_policy_two_stage_launches counts the reductions that took
 * the two-stage form, in the plan and here. */
int64_t pvr_debug_policy_two_stage_launches(void);
/* out0[c] (and out1[c] when out1 != NULL) = sum_r X[r][c], X [R][C] */
pvr_status pvr_op_policy_colsum(const float *X, float *out0, float *out1, int32_t R, int32_t C, int32_t form, void *hip_stream);
/* Training-mode BatchNorm1d statistics of X [R][C] as the forward takes them: mean = colsum / n_global, sumsq = sum_r (x - mean)^2,
 * invstd = 1 / sqrt(sumsq / n_global + 1e-5), running_mean / running_var updated in place with momentum 0.1 (the unbiased variance
 * sumsq / (n_global - 1) goes into running_var), *num_batches_tracked += 1 (may be NULL).  n_global = R, or the global row count under SyncBN. */
pvr_status pvr_op_policy_bn_stats(const float *X, int32_t R, int32_t C, float n_global, int32_t form, float *mean, float *invstd, float *sumsq,
                                  float *running_mean, float *running_var, int64_t *num_batches_tracked, void *hip_stream);
/* y = (x - mean) * invstd * gamma + beta; is_var != 0: the third argument is a variance (eval mode), invstd = 1 / sqrt(var + 1e-5).  C % 4 == 0 */
pvr_status pvr_op_policy_bn_apply(const float *x, const float *mean, const float *invstd_or_var, const float *gamma, const float *beta, float *y,
                                  int32_t R, int32_t C, int32_t is_var, void *hip_stream);
/* dgamma[c] = sum_r dY (X - mean) invstd, dbeta[c] = sum_r dY */
pvr_status pvr_op_policy_bn_backward_sums(const float *X, const float *dY, const float *mean, const float *invstd, float *dgamma, float *dbeta,
                                          int32_t R, int32_t C, int32_t form, void *hip_stream);
/* xhat = (x - mean) * invstd.  C % 4 == 0 */
pvr_status pvr_op_policy_bn_xhat(const float *x, const float *mean, const float *invstd, float *xhat, int32_t R, int32_t C, void *hip_stream);
/* The fold of the BatchNorm affine gradients into fc1's weight gradient: S_dW [H][O] holds S = dz1^T xhat on entry and dW1 = gamma S + beta db1^T on
 * return; dgamma[c] = sum_j W1[j][c] S[j][c], dbeta[c] = sum_j W1[j][c] db1[j].  O % 128 == 0 */
pvr_status pvr_op_policy_bn_fold(float *S_dW, const float *W1, const float *db1, const float *gamma, const float *beta, float *dgamma, float *dbeta,
                                 int32_t H, int32_t O, void *hip_stream);
/* dx = gamma invstd (dy - dbeta / n_stat - xhat dgamma / n_stat): from x (xhat formed inside), or in place on dx = dy from a stored xhat (C % 4 == 0) */
pvr_status pvr_op_policy_bn_dx(const float *x, const float *dy, const float *mean, const float *invstd, const float *gamma, const float *dgamma,
                               const float *dbeta, float *dx, int32_t R, int32_t C, int32_t n_stat, void *hip_stream);
pvr_status pvr_op_policy_bn_dx_xhat(float *dx, const float *xhat, const float *invstd, const float *gamma, const float *dgamma, const float *dbeta,
                                    int32_t R, int32_t C, int32_t n_stat, void *hip_stream);
/* nd = |1 - (done != 0)|;  out[t][b][:] = nd[t][b] * (t == 0 ? h_init[b] : hs[t-1][b]) (hs (T,B,H), h_init (B,H));  out [N][16] = in [N][A] zero-padded;
 * out[0] = (fixed-order sum of loss_row[0..n)) / n */
pvr_status pvr_op_policy_notdone(const uint8_t *done, float *nd, int32_t n, void *hip_stream);
pvr_status pvr_op_policy_hprev(const float *hs, const float *h_init, const float *nd, float *out, int32_t T, int32_t B, int32_t H, void *hip_stream);
pvr_status pvr_op_policy_dlogits_pad(const float *in, float *out, int32_t N, int32_t A, void *hip_stream);
pvr_status pvr_op_policy_loss_mean(const float *loss_row, int32_t n, float *out, void *hip_stream);
/* One step of one LSTM layer (the per-step launch).  G [B][4H] holds the input projection with b_ih on entry and the activated gates i,f,g,o on return;
 * gates = G + b_hh + (nd * h_prev) W_hh^T, c_out = f (nd * c_prev) + i g, h_out = o tanh(c_out).  H a multiple of 1024 */
pvr_status pvr_op_policy_lstm_fwd_step(float *G, const float *h_prev, const float *c_prev, const float *nd, const float *W_hh, const float *b_hh,
                                       float *h_out, float *c_out, int32_t B, int32_t H, void *hip_stream);
/* One BPTT step of one layer (the two per-step launches).  G [B][4H]: activated gates of step t in, gate gradients dG out; dc_carry [B][H] in / out.
 * dh = dh_ext + nd_next * (dG_next W_hh), the recurrent product through partial ([16][B][H] scratch); dG_next == NULL is step T-1: no recurrent
 * term, dc_carry is not read, W_hh / nd_next / partial may be NULL. */
pvr_status pvr_op_policy_lstm_bwd_step(const float *dG_next, const float *W_hh, const float *nd_next, const float *dh_ext, float *dc_carry, float *G,
                                       const float *c_t, const float *c_prev, const float *nd, float *partial, int32_t B, int32_t H, void *hip_stream);
/* Heads + BC loss: logits [N][A], baseline [N], action [N] = argmax (first index on ties); with target != NULL also loss_row [N] (NaN for a target
 * outside [0, A)) and dlogits [N][16] = (softmax - onehot) / N, columns A..15 zero.  Without a target loss_row and dlogits may be NULL. */
pvr_status pvr_op_policy_heads(const float *out, const float *Wp, const float *bp, const float *Wb, const float *bb, const int64_t *target,
                               float *logits, float *baseline, int64_t *action, float *loss_row, float *dlogits, int32_t N, int32_t H, int32_t A,
                               void *hip_stream);
/* dWp [A][H] = dlogits^T out, dbp [A] = column sums of dlogits (form as above), dout [N][H] = dlogits Wp.  dlogits is the padded [N][16] */
pvr_status pvr_op_policy_head_backward(const float *dlogits, const float *out, const float *Wp, float *dWp, float *dbp, float *dout, int32_t N,
                                       int32_t H, int32_t A, int32_t form, void *hip_stream);

/* How every fp32 GEMM of the policy is computed (process-wide; the reference's counterpart is torch's fp32 matmul, src/models.py:66-73):
 *   0  fp32 MFMA (v_mfma_f32_16x16x4_f32: the ascending-k fma chain; the default, rounds 1-3)
 *   1  bf16 MFMA on an exact three-term split of both operands, six products per pair, fp32 accumulation (round 3, opt-in: 2.7 x closer
 *      to an fp64 product than mode 0 and about as fast); 2 / 3: the same with 128 x 128 / 64 x 64 tiles forced
 *  -1  back to the default (environment PVR_GEMM_BF16X3, else 0) */
pvr_status pvr_debug_set_gemm_mode(int32_t mode);

#ifdef __cplusplus
}
#endif
#endif /* PVR_POLICY_H */
