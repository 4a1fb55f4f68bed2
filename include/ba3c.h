/*
 * ba3c.h — C ABI of the MI355X-native BA3C learner/predictor hot path (libba3c.so).
 *
 * Plain pointers and sizes only: every data buffer is owned by the caller (the Python
 * host allocates them with PyTorch-ROCm); the handle owns static configuration, a few HIP
 * events and a few KB of device memory allocated by ba3c_create (the tagged-partial words of
 * the fused clip + optimizer launch and of the one-launch bucket clip, the chained launches'
 * signal counters; without a device they stay unallocated and those launches fall back to
 * unchained ones).  One handle serves one stream at a time.  No other call allocates
 * device memory, none synchronises the stream except ba3c_probe_read, and none throws:
 * every entry returns a BA3C_* status and
 * ba3c_last_error() holds a thread-local message.  All device pointers must be 16-byte
 * aligned.  `stream` is a hipStream_t (NULL = default stream).
 *
 * Each entry point replaces one piece of the reference TF-1.2 graph / runtime
 * (paths relative to /root/reference/src):
 *   ba3c_forward        OpenAIGym/train.py:164-299 for is_training=False (towerp0:
 *                       'logitsT', 'pred_value'), served by OnlinePredictor._do_call
 *                       tensorpack_cpu/tensorpack/predict/base.py:80-92 and
 *                       MultiThreadAsyncPredictor predict/concurrency.py:172-219
 *   ba3c_train_grads    OpenAIGym/train.py:164-327 forward + A3C loss and TF autodiff
 *                       tensorpack_cpu/tensorpack/train/multigpu.py:85-86
 *   ba3c_clip_grads     OpenAIGym/train.py:329-330 MapGradient(clip_by_average_norm(.,0.1)),
 *                       applied per replica in train/base.py:206-217, multigpu.py:157
 *   ba3c_apply_update   OpenAIGym/train.py:582-597 optimizer.apply_gradients
 *                       (multigpu.py:194): Adam / RMSProp / GD / Momentum / Adagrad / Adadelta
 *   ba3c_sample         OpenAIGym/train.py:382 np.random.choice(len(p), p=p) given its draw u
 *   (gradient mean)     OpenAIGym/train.py:598-606 SyncReplicasOptimizer: the host
 *                       all-reduces the clipped flat gradient buffer over RCCL between
 *                       ba3c_clip_grads and ba3c_apply_update (grad_scale = 1/world).
 */
#ifndef BA3C_H
#define BA3C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BA3C_OK 0
#define BA3C_ERR_INVALID 1  /* bad argument / shape / config */
#define BA3C_ERR_HIP 2      /* a HIP runtime call failed */

/* optimizer ids (OpenAIGym/train.py:583-597, run_job.py -o choices) */
#define BA3C_OPT_ADAM 0
#define BA3C_OPT_GD 1
#define BA3C_OPT_ADAGRAD 2
#define BA3C_OPT_ADADELTA 3
#define BA3C_OPT_MOMENTUM 4
#define BA3C_OPT_RMS 5

/* scalars written by ba3c_train_grads (double[BA3C_NUM_SCALARS]); names are the
 * TfDictOp keys of train/multigpu.py:193-205 */
#define BA3C_SC_COST 0
#define BA3C_SC_POLICY_LOSS 1    /* policy_loss*128/B              train.py:311 */
#define BA3C_SC_XENTROPY_LOSS 2  /* xentropy_loss*128/B*beta       train.py:315-316 */
#define BA3C_SC_VALUE_LOSS 3     /* value_loss*128/B               train.py:320 */
#define BA3C_SC_ADVANTAGE 4      /* mean(stop_grad(V)-R)           train.py:323 */
#define BA3C_SC_PRED_REWARD 5    /* mean(V)                        train.py:321 */
#define BA3C_SC_MAX_LOGIT 6      /* max(softmax)                   train.py:291 */
#define BA3C_SC_ACTIVE_RELUS 7   /* sum count_nonzero(relu outs)   train.py:271 */
#define BA3C_NUM_SCALARS 8

/* kernel ids for the timing probe */
#define BA3C_K_CONV0_FWD 0
#define BA3C_K_CONV1_FWD 1
#define BA3C_K_CONV2_FWD 2
#define BA3C_K_CONV3_FWD 3
#define BA3C_K_FC1_FWD 4
#define BA3C_K_HEADS 5
#define BA3C_K_FC1_DGRAD 6
#define BA3C_K_CONV3_DGRAD 7
#define BA3C_K_CONV2_DGRAD 8
#define BA3C_K_CONV1_DGRAD 9
#define BA3C_K_HEAD_WGRAD 10
#define BA3C_K_FC1_WGRAD 11
#define BA3C_K_CONV3_WGRAD 12
#define BA3C_K_CONV2_WGRAD 13
#define BA3C_K_CONV1_WGRAD 14
#define BA3C_K_CONV0_WGRAD 15
#define BA3C_K_WGRAD_REDUCE 16
#define BA3C_K_CLIP 17
#define BA3C_K_UPDATE 18
#define BA3C_K_SCALARS 19   /* TfDictOp scalar reduction (its own launch or a job of conv3's input-gradient launch) */
#define BA3C_NUM_KERNELS 20

typedef struct ba3c_handle ba3c_handle;

/* Network geometry — the flag surface of OpenAIGym/parse.py:9-70 / run_job.py:13-48. */
typedef struct ba3c_config {
  int32_t max_batch;         /* largest B any call on this handle passes (workspace sizing) */
  int32_t channels;          /* real input channels C = 4*--channels (4 or 12), train.py:95 */
  int32_t fc_neurons;        /* --fc_neurons F (multiple of 4*fc_splits) */
  int32_t fc_splits;         /* --fc_splits S  (train.py:216-229) */
  int32_t num_actions;       /* A = env action count (train.py:122), 1..31 */
  int32_t replace_with_conv; /* 1: --replace_with_conv True (default); 0: --use_normal_fc */
  int32_t ps;                /* --ps: number of legacy FC splits (train.py:230-243) */
} ba3c_config;

/* Hyper-parameters of one optimizer apply. Power terms are the TF float32 variables
 * beta1_power/beta2_power BEFORE this apply (beta^t at step t). */
typedef struct ba3c_opt_params {
  float lr, beta1, beta2, epsilon;    /* Adam (train.py:584) */
  float beta1_power, beta2_power;     /* Adam bias-correction state */
  float decay, momentum;              /* RMSProp (TF defaults 0.9 / 0.0), Momentum 0.9 */
  float rho;                          /* Adadelta (0.95) */
} ba3c_opt_params;

int ba3c_create(const ba3c_config* cfg, ba3c_handle** out);
void ba3c_destroy(ba3c_handle* h);
const char* ba3c_last_error(void);
int ba3c_version(void);

/* Flat parameter layout shared by params / grads / optimizer slots.  Tensor i is
 * name (checkpoint key, e.g. "conv0/W"), at float offset `offset`, `numel` elements in
 * TF layout (HWIO conv, [in,out] FC).  Offsets are 64-float aligned; gaps are zero. */
int ba3c_num_tensors(const ba3c_handle* h);
int ba3c_tensor_info(const ba3c_handle* h, int32_t i, const char** name, int64_t* offset,
                     int64_t* numel, int32_t shape[4], int32_t* ndim);
int64_t ba3c_flat_size(const ba3c_handle* h);
/* Bytes of scratch device memory a call with batch B needs (train=1: ba3c_train_grads). */
size_t ba3c_workspace_size(const ba3c_handle* h, int32_t batch, int32_t train);
/* Introspection of the workspace a call with batch B carved (for tests / debugging): byte
 * offset and size of an intermediate — "p0","p1","p2" pooled maps [B,H,W,C] fp32, "c0".."c2"
 * argmax codes (uint8, 0..3 = first max of the 2x2 window, 255 = max <= 0), "a3" [B,1600],
 * "h" [B,F], and in training "dh","dy3","dp2","dp1","dp0" gradients. */
int ba3c_workspace_tensor(const ba3c_handle* h, int32_t batch, int32_t train, const char* name,
                          int64_t* offset_bytes, int64_t* bytes);

/* Predictor: one forward of B uint8 [B,84,84,C] states.  probs = softmax(policy)
 * ('logits', train.py:288), probsT = softmax(policy*explore_factor) ('logitsT', :299),
 * value = 'pred_value' [B].  Any output pointer may be NULL. */
int ba3c_forward(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                 int32_t batch, float explore_factor, void* workspace, float* probs,
                 float* probsT, float* value);

/* Learner: forward + A3C loss + backward for one tower.  Writes RAW (unclipped) gradients
 * of every tensor into `grads` (flat layout, fully overwritten incl. gaps) and
 * BA3C_NUM_SCALARS doubles into `scalars` (device memory, may be NULL).
 * action: int64 [B] in [0,A); futurereward: fp32 [B]. */
int ba3c_train_grads(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                     const int64_t* action, const float* futurereward, int32_t batch,
                     float entropy_beta, void* workspace, float* grads, double* scalars);

/* ba3c_train_grads in two phases for data-parallel bucketing: phase 1 runs the
 * forward, the loss / scalars and the backward of the heads and fc1 and leaves THEIR gradient
 * tensors (tensors ba3c_bucket_tensor(h) .. end of the flat layout) final; phase 2 (same
 * arguments, same workspace) runs conv3..conv0 and finishes the rest.  Phase 0 = both = the
 * bit-identical ba3c_train_grads.  Between the phases the caller may clip and all-reduce the
 * fc1 + heads bucket while the conv layers run (the reference's per-variable PS pushes,
 * OpenAIGym/train.py:598-606).  Any other phase is refused with BA3C_ERR_INVALID before anything
 * is launched. */
int ba3c_train_grads_phase(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                           const int64_t* action, const float* futurereward, int32_t batch,
                           float entropy_beta, void* workspace, float* grads, double* scalars,
                           int32_t phase);
/* ba3c_train_grads_phase with the clipped-surrogate (PPO, Schulman et al. 2017) policy term in
 * place of the A3C one; every other launch, the phases 0-2 and their meaning, the scalars and
 * their scaling are ba3c_train_grads_phase's (the heads run in phase 1).
 * rows: fp32 [B][4], row n = {R, V_old, l_old, w} — the return (the value target, the A3C
 * futurereward), the predictor's value when the action was taken, l_old =
 * log(pi_old(a) + 1e-6) (ba3c_sample_logp) and a caller-supplied advantage (read only with
 * BA3C_PPO_ADV_FROM_ROW).  With p = softmax(z), lp = log(p + 1e-6) and the current value V:
 *   Adv  = R - V_old                                   (a constant of the sample)
 *   rho  = exp(lp[a] - l_old)
 *   s    = -min(rho Adv, clip(rho, 1 - clip_eps, 1 + clip_eps) Adv)
 *   cost = (sum_n s + entropy_beta sum_n sum_k p_k lp_k + 1/2 sum_n (V - R)^2) / B
 * and its gradient is the A3C one with the advantage factor replaced by
 *   c = (rho Adv <= clip(rho, ...) Adv) ? -Adv rho : 0        (a tie takes the unclipped branch);
 * at rho = 1 and V_old = V it is ba3c_train_grads' gradient.  scalars[1] (policy_loss) is
 * sum_n s * 128 / B; scalars[4] (advantage) stays mean(V - R) with the current V.
 * ratio: fp32 [B] device memory, receives rho per sample; may be NULL.
 * The two further pieces every PPO implementation carries (baselines ppo2, CleanRL), both off
 * at 0:
 *   flags & BA3C_PPO_ADV_FROM_ROW: Adv = rows[n][3] (ba3c_ppo_norm_adv writes it) instead of
 *     R - V_old, in s and in c; R and V_old keep their other uses.
 *   vclip_eps > 0: with d = V - V_old and Vc = V_old + sign(d) vclip_eps,
 *     use_clipped = |d| > vclip_eps and (Vc - R)^2 > (V - R)^2      (a tie is unclipped)
 *     and the value term of the cost and scalars[3] (value_loss) take (Vc - R)^2 where
 *     use_clipped, else (V - R)^2, i.e. 1/2 max((V - R)^2, (Vc - R)^2) per sample; dV is 0 where
 *     use_clipped, else (V - R) / B.  scalars[4] stays mean(V - R).  vclip_eps = 0: no clipping.
 * Refused with BA3C_ERR_INVALID before any GPU call, in this order: rows NULL or not 16-byte
 * aligned, ratio given but not 16-byte aligned, clip_eps not in (0, 1) (a NaN included),
 * vclip_eps negative or not finite (a NaN included), flags with a bit other than
 * BA3C_PPO_ADV_FROM_ROW, phase outside 0..2, then ba3c_train_grads_phase's checks. */
#define BA3C_PPO_ADV_FROM_ROW 1u
int ba3c_train_grads_ppo_ext(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                             const int64_t* action, const float* rows, int32_t batch,
                             float entropy_beta, float clip_eps, float vclip_eps, uint32_t flags,
                             void* workspace, float* grads, double* scalars, float* ratio,
                             int32_t phase);
/* ba3c_train_grads_ppo_ext with vclip_eps = 0 and flags = 0: the same call, launches, outputs and
 * refusals (rows[n][3] is not read). */
int ba3c_train_grads_ppo(ba3c_handle* h, void* stream, const float* params, const uint8_t* state,
                         const int64_t* action, const float* rows, int32_t batch,
                         float entropy_beta, float clip_eps, void* workspace, float* grads,
                         double* scalars, float* ratio, int32_t phase);
/* Per-minibatch advantage normalisation, in place on the n rows {R, V_old, l_old, .} of a PPO
 * step (fp32 [n][4], device): with Adv_i = (double)R_i - (double)V_old_i, mean = sum Adv / n and
 * the population std = sqrt(sum (Adv - mean)^2 / n) (two passes, fp64),
 *   rows[i][3] = (float)((Adv_i - mean) / (std + 1e-8));
 * columns 0-2 are not written.  stats (device, 8-byte aligned, may be NULL) receives
 * {mean, std} as doubles.  One launch of one workgroup; the sums run in a fixed order, so the
 * result is a function of the rows alone (a repeat gives the same bits).
 * Refused with BA3C_ERR_INVALID before any GPU call: rows NULL or not 16-byte aligned, stats not
 * 8-byte aligned, n < 1. */
int ba3c_ppo_norm_adv(void* stream, float* rows, int32_t n, double* stats);
/* Record the HIP event `event` (a hipEvent_t of the caller's, NULL: none) on the pass's stream
 * in every later phase-2 pass, right after conv3's input- and weight-gradient launches (the
 * event only has to follow phase 1): the N>1 step starts the fc1 + heads
 * bucket's exchange from there, so its collective's workgroups take CUs at the boundary before
 * conv2's launch (short, non-persistent workgroups the dispatcher rebalances) instead of
 * beside conv3's persistent ones. */
int ba3c_set_phase2_event(ba3c_handle* h, void* event);
/* First tensor of the fc1 + heads bucket (tensors before it: the conv layers). */
int ba3c_bucket_tensor(const ba3c_handle* h);

/* Per-tensor tf.clip_by_average_norm(g, 0.1) in place (n = graph numel incl. padding). */
int ba3c_clip_grads(ba3c_handle* h, void* stream, float* grads, void* workspace);
/* The same clip over tensors [t0, t1) only (a bucket): one launch with tagged partials when
 * the bucket's chunks fit one workgroup per CU (BA3C_FUSED_UPDATE on), else the sum-of-squares
 * + clip launches; bit-identical. */
int ba3c_clip_grads_range(ba3c_handle* h, void* stream, float* grads, void* workspace, int32_t t0,
                          int32_t t1);
/* Clip of the whole gradient's norm (tf.clip_by_global_norm, torch's clip_grad_norm_, up to
 * rounding; the rule is stated in ba3c_amd/gradclip.py), in place over every tensor of the flat
 * buffer; it replaces ba3c_clip_grads, it does not follow it:
 *   norm = sqrt(sum of (double)g^2 over every element of every tensor)   (alignment gaps: not elements)
 *   f    = norm > max_norm ? max_norm / norm : 1.0      (double; a NaN norm leaves f = 1.0)
 *   g    = (float)((double)g * f)                       (f == 1.0: g keeps its bits)
 * Two plain launches, no in-launch waits and no atomics; the sums run in a fixed order, so a
 * repeat gives the same bits.  scratch: device memory of the caller's, 8-byte aligned, of
 * scratch_doubles >= ba3c_global_clip_scratch(h) = nchunks + 2 doubles; after the call
 * scratch[nchunks] = norm and scratch[nchunks + 1] = f.  The workspace is not touched.
 * Refused with BA3C_ERR_INVALID before any launch, the first failure reported: a null handle;
 * grads NULL or not 16-byte aligned; max_norm not finite or not > 0 (a NaN included); scratch
 * NULL or not 8-byte aligned; scratch_doubles < nchunks + 2. */
int64_t ba3c_global_clip_scratch(const ba3c_handle* h);     /* host only */
int ba3c_clip_grads_global(ba3c_handle* h, void* stream, float* grads, double max_norm,
                           double* scratch, int64_t scratch_doubles);

/* One optimizer apply over the flat buffers: g_eff = grads*grad_scale (1/world after an
 * all-reduce-sum), or, with fuse_clip=1, clip_by_average_norm(grads) fused in (single
 * replica; one launch with a grid barrier when the tensor chunks fit one workgroup per CU,
 * bit-identical to ba3c_clip_grads followed by an unfused apply).  slot0/slot1: Adam m/v,
 * RMS ms/mom, Adagrad accum, Adadelta accum/accum_update, Momentum accum; unused slots may
 * be NULL. */
int ba3c_apply_update(ba3c_handle* h, void* stream, int32_t opt, float* params,
                      const float* grads, float* slot0, float* slot1,
                      const ba3c_opt_params* hp, float grad_scale, int32_t fuse_clip,
                      void* workspace);

/* Same apply with the Adam bias-correction state on the device: dev_powers = {beta1_power,
 * beta2_power} (float32, TF's variables) is read by the update and multiplied by
 * (beta1, beta2) after it, on the stream — so a captured hipGraph of the whole step replays
 * with the correct per-step alpha.  hp->beta*_power are ignored. */
int ba3c_apply_update_dev(ba3c_handle* h, void* stream, int32_t opt, float* params,
                          const float* grads, float* slot0, float* slot1,
                          const ba3c_opt_params* hp, float* dev_powers, float grad_scale,
                          int32_t fuse_clip, void* workspace);

/* Action sampling: actions[i] = #{k : cdf_i[k] <= u[i]} with cdf_i = cumsum(double(p_i))
 * / cdf_i[A-1]  (numpy RandomState.choice).  nonfinite (device int32, may be NULL) is
 * set to 1 if any probability is not finite (train.py:381 assert). */
int ba3c_sample(void* stream, const float* probs, const double* u, int32_t batch,
                int32_t num_actions, int64_t* actions, int32_t* nonfinite);

/* ba3c_sample that also records the behaviour policy's log-probability of the drawn action:
 * actions and nonfinite are exactly ba3c_sample(probs, u, ...)'s, and
 * logp[i] = (float) log((double) pi[i][min(actions[i], A-1)] + 1e-6)  (fp32 [B], device).
 * probs is the distribution sampled from ('logitsT'), pi the one whose log is recorded
 * ('logits', the l_old of ba3c_train_grads_ppo's rows); they may be the same pointer. */
int ba3c_sample_logp(void* stream, const float* probs, const float* pi, const double* u,
                     int32_t batch, int32_t num_actions, int64_t* actions, float* logp,
                     int32_t* nonfinite);

/* Evaluation action (OpenAIGym/common.py:24-33, play_one_episode): actions[i] = first argmax of
 * probs[i] (np.argmax), or random_actions[i] (the player's action_space.sample()) when
 * u[i] < eps (`random.random() < 0.001`). */
int ba3c_greedy(void* stream, const float* probs, const double* u, const int64_t* random_actions,
                int32_t batch, int32_t num_actions, double eps, int64_t* actions);

/* Timing probe: bracket every launch of kernel `kernel_id` with HIP events (on the stream
 * it is launched on) until disabled (kernel_id = -1).  ba3c_probe_read synchronises the
 * recorded events and returns the summed milliseconds and launch count since enabling. */
int ba3c_probe_enable(ba3c_handle* h, int32_t kernel_id);
/* Device-side error flags of the handle's in-launch waits (bit 0: a fused clip+optimizer launch,
 * bit 1: a one-launch ba3c_clip_grads_range, stopped waiting for another workgroup's partial;
 * bit 2: a chained launch's conv0 workgroups stopped waiting for the zeroing of the ReLU
 * counters / max slots — the results are invalid).  0 in normal operation.  Synchronises the
 * device (diagnostics / tests only).  Once bit 2 is seen the handle zeroes its chain words and
 * stops chaining launches (the flag stays set). */
int ba3c_device_errors(ba3c_handle* h, uint32_t* flags);

int ba3c_probe_read(ba3c_handle* h, double* total_ms, int32_t* launches);
/* Bracket only the first of every `n` launches of the probed kernel (default 1: every launch),
 * counted from here / from ba3c_probe_enable.  Each bracket's two events leave 5-6 us gaps in
 * the stream, so a throughput run samples its launches (bench.py --probe-every). */
int ba3c_probe_every(ba3c_handle* h, int32_t n);
/* The synchronous gradient exchange through the C ABI (SURVEY.md §8b `ba3c_allreduce_mean`;
 * replaces the SyncReplicasOptimizer aggregation on the parameter servers,
 * OpenAIGym/train.py:598-606): an RCCL communicator owned by the handle.  RCCL is resolved at
 * run time from the process's librccl.so.1 (torch's copy when torch is loaded).
 * ba3c_comm_unique_id: rank 0 draws BA3C_UNIQUE_ID_BYTES bytes and the caller broadcasts them;
 * ba3c_comm_init is collective over the ranks; ba3c_comm_destroy(abort = 1) does not wait for
 * enqueued collectives (an exit path where a peer may be gone).  ba3c_allreduce_sum sums
 * `count` floats in place over the ranks on `stream`; ba3c_allreduce_mean also scales them by
 * 1/nranks (16-byte aligned `grads`).  The Python trainer drives the same RCCL through
 * ba3c_amd/rccl.py, with the same semantics. */
#define BA3C_UNIQUE_ID_BYTES 128
int ba3c_comm_unique_id(void* id_out);
int ba3c_comm_init(ba3c_handle* h, const void* id, int32_t nranks, int32_t rank);
int ba3c_comm_destroy(ba3c_handle* h, int32_t abort);
int ba3c_allreduce_sum(ba3c_handle* h, void* stream, float* buf, int64_t count);
int ba3c_allreduce_mean(ba3c_handle* h, void* stream, float* grads, int64_t count);
/* Diagnostic, not part of the reference's interface: enqueue on `stream` a launch of `n_cus`
 * workgroups that each hold one whole CU (all 160 KiB of its LDS) for `usec` microseconds,
 * doing nothing.  bench.py --occupy uses it on the exchange stream to stand in for RCCL's
 * channel workgroups while the conv backward runs (how persistent kernels degrade when K CUs
 * are missing). */
int ba3c_occupy_cus(void* stream, int32_t n_cus, double usec);

/* Arithmetic path of kernel `kernel_id` on this handle (for roofline accounting; no
 * reference counterpart): the number of 16-bit MFMA products it issues per fp32 product —
 * 6 for the bf16 hi/mid/lo split, 3 for the scaled fp16 hi/lo split (or conv0's u8 x bf16x3),
 * 2 for conv0's u8 x scaled-fp16 hi/lo — or 1 for fp32 MFMA (v_mfma_f32_*_f32), 0 for a
 * kernel with no matrix work; -1 on a bad id. */
int ba3c_kernel_split(const ba3c_handle* h, int32_t kernel_id);

/* Operand family of a split kernel: 3 = bf16 planes (v_mfma_*_bf16), 2 = power-of-two
 * scaled fp16 planes (v_mfma_*_f16); otherwise the value of ba3c_kernel_split (1, 0, -1). */
int ba3c_kernel_family(const ba3c_handle* h, int32_t kernel_id);

/* Kernels that ran inside kernel `kernel_id`'s launch in the last training pass (multi-job
 * launches: the probe of `kernel_id` brackets them too, and they record no launch of their own),
 * as a bitmask of kernel ids; 0 when the launch ran only that kernel, -1 on a bad id.  For
 * roofline accounting only (no reference counterpart).
 *
 * One forward launch merges kernels as well, in ba3c_train_grads and ba3c_forward alike: with
 * channels == 4, at the batches where conv1's forward runs as the ring walk (batch >= 2 x CUs
 * and (batch % (2 x CUs) == 0 or batch >= 16 x CUs)), conv0's and conv1's forward are ONE
 * persistent launch of 2 x CUs workgroups.  Each workgroup takes its own contiguous images
 * through conv0 and then conv1, image by image, and waits for no other workgroup; the results
 * are bit for bit those of the two launches.  It is timed under BA3C_K_CONV0_FWD, whose mask
 * then holds BA3C_K_CONV1_FWD's bit (after ba3c_forward too), and BA3C_K_CONV1_FWD records no
 * launch.  BA3C_FWD01=0 in the environment of ba3c_create keeps the two launches (any value but
 * 0 or 1 is rejected, like the other launch-structure switches); every other batch,
 * BA3C_RING=0 and BA3C_GENERIC=1 run them as before. */
int ba3c_kernel_merged(const ba3c_handle* h, int32_t kernel_id);

/* ---- data formats either side of the path ---------------- */

/* n-step returns of MySimulatorMaster (OpenAIGym/train.py:408-437, _parse_memory) for n_envs
 * simulators at once.  Env e's memory is a ring of `slots` transitions (i-th oldest at slot
 * (start[e]+i) % slots), length[e] of them with known rewards (float64, as gym returns them)
 * and predictor values.  not over: the newest transition only bootstraps (R = its value) and
 * is not emitted; over: R = 0 and all are emitted.  Emitted in reverse time order, env by env
 * (the reference's queue order): R = clip(r,-1,1) + gamma*R in float64, stored as float32;
 * src[i] = e*slots + slot of datapoint i; init_R / over as the reference's datapoint
 * fields.  Output arrays hold n_envs*slots entries; *count (device int32) receives the
 * number written.  One workgroup: latency-bound. */
int ba3c_nstep_returns(void* stream, const double* reward, const float* value,
                       const int32_t* start, const int32_t* length, const uint8_t* is_over,
                       int32_t n_envs, int32_t slots, double gamma, float* R, int32_t* src,
                       float* init_R, uint8_t* over, int32_t* count);

/* lambda-returns over the same memories: ring layout, outputs, emission order and the
 * over / not-over rule are those of ba3c_nstep_returns; only the recursion differs.  Per
 * simulator, in reverse time order over the emitted transitions, in float64:
 *   R = clip(r,-1,1) + gamma * ((1 - lambda) * Vnext + lambda * R)
 * where R and Vnext start at the bootstrap (the newest transition's value when not over, 0
 * when over) and Vnext then is the value of the transition emitted before (the next one in
 * time).  Every product and sum rounds once (no fused multiply-add), R is stored as float32.
 * R - value is the GAE(lambda) advantage sum_k (gamma*lambda)^k delta_{t+k}; lambda = 1 is the
 * recursion of ba3c_nstep_returns exactly, lambda = 0 is clip(r) + gamma * Vnext.
 * 1 <= slots <= 129; lambda in [0, 1] and gamma in (0, 1] (NaN is rejected), checked with the
 * pointers before any GPU call.  One workgroup per 32 simulators, none waiting for another:
 * each sums the emitted counts before it for its output offset. */
int ba3c_lambda_returns(void* stream, const double* reward, const float* value,
                        const int32_t* start, const int32_t* length, const uint8_t* is_over,
                        int32_t n_envs, int32_t slots, double gamma, double lambda, float* R,
                        int32_t* src, float* init_R, uint8_t* over, int32_t* count);

/* BatchData / EnqueueThread hand-off (dataflow/common.py:64-99, train/trainer.py:116-155):
 * out[i] = rows[idx[i]] for n rows (any 0 <= n <= INT32_MAX) of row_bytes (a multiple of 16,
 * e.g. 84*84*C states, or exactly 8: int64 actions). */
int ba3c_gather_rows(void* stream, const void* rows, const int32_t* idx, int32_t n,
                     int64_t row_bytes, void* out);

/* HistoryFramePlayer (RL/history.py:12-55) for n_envs simulators: state[e] ([pixels][hist_len
 * * channels] uint8, oldest frame first) becomes concat(state[..., channels:], frame[e]); when
 * is_over[e] (may be NULL) the frame starts a new episode: zeros + frame. */
int ba3c_history_push(void* stream, const uint8_t* frame, uint8_t* state, const uint8_t* is_over,
                      int32_t n_envs, int32_t pixels, int32_t hist_len, int32_t channels);

/* The episodes the training simulators finish (MySimulatorMaster's self.stats[ident] fed to
 * self.games at every episode end, OpenAIGym/train.py:394-412), for n_envs simulators in one
 * launch; ba3c_amd/episodes.py (update_numpy) is the bit-exact statement.  For every e:
 *   ret[e] += reward[e] (float64, one rounding; the raw, unclipped reward);  len[e] += 1
 *   where over[e]: ring slot (*head + k) % cap, k = the number of e' < e with over[e'] in this
 *     launch, receives log_score = ret[e], log_len = len[e], log_env = e; then ret[e] = +0.0
 *     and len[e] = 0
 *   *head += the number of e with over[e]
 * so one launch's episodes are logged in increasing e (a scan over the flags, no atomics: two
 * runs log identical rings).  *head (device int64, episodes ever logged) is read and written by
 * the device only; the host reads it when it drains the ring.  Refused before any launch, in
 * this order (BA3C_ERR_INVALID): a null pointer (all are required); n_envs < 1; cap < n_envs
 * (one launch must never overwrite its own entries); reward / ret / log_score / head not
 * 8-byte or len / log_len / log_env not 4-byte aligned.  Never synchronises, never allocates.
 * One workgroup: latency-bound (21 bytes per simulator). */
int ba3c_episode_stats(void* stream, const double* reward, const uint8_t* over, int32_t n_envs,
                       double* ret, int32_t* len, double* log_score, int32_t* log_len,
                       int32_t* log_env, int32_t cap, int64_t* head);

/* ---- GridBreakout: an on-device game (stands in for RL/gymenv.py + the 84x84 resize) ----- */

/* A small integer-only Breakout for n_envs simulators; ba3c_amd/breakout.py states the rules
 * (constants, step_numpy, render_numpy) and is the oracle of these entry points.  All game
 * state is int32, one 64-byte (16-byte aligned) row per simulator:
 *   game[e] = [px, bx, by, vx, vy, in_play, lives, score, t, rng, b0, b1, b2, b3, b4, b5]
 * px: paddle left edge (0..72); (bx, by): the 2x2 ball's top-left; (vx, vy): its velocity;
 * in_play: 0 until FIRE serves; lives: 5 per episode; score / t: reward sum and steps of the
 * episode; rng: the serve LCG's uint32 bits; b_r: 14-bit mask of row r's live bricks.
 *
 * ba3c_breakout_step applies action[e] (0 NOOP, 1 FIRE, 2 RIGHT, 3 LEFT, anything else NOOP;
 * the value is compared, never used as an index) to every simulator and writes reward[e]
 * (float64, as gym returns it), over[e], and ep_score[e] ONLY where over[e] (the finished
 * episode's score; the row is then already reset, GymEnv's auto-restart).  An episode ends
 * when lives reach 0, no brick is left, or t >= limit (LimitLengthPlayer).  The frame after
 * the step (on over: the new episode's first) is rendered to frame[e] ([84*84] uint8, may be
 * NULL) and, when state is given ([84*84][4] uint8, may be NULL), pushed into the H=4, c=1
 * frame history in the same launch: per pixel dword (old >> 8) | (pix << 24), old = 0 where
 * over[e] — bit-identical to ba3c_history_push(frame, state, over).
 *
 * ba3c_breakout_render renders the current rows without stepping; with state it starts the
 * history (zeros + frame).
 *
 * Both validate their arguments on the host (null game / action / outputs, n_envs < 1,
 * limit < 1, misaligned game / state / frame -> BA3C_ERR_INVALID) before touching the
 * device, never synchronise and never allocate.  One launch, one 256-thread workgroup per
 * simulator. */
int ba3c_breakout_step(void* stream, int32_t* game, const int64_t* action, int32_t n_envs,
                       int32_t limit, double* reward, uint8_t* over, int32_t* ep_score,
                       uint8_t* frame, uint8_t* state);
int ba3c_breakout_render(void* stream, const int32_t* game, int32_t n_envs, uint8_t* frame,
                         uint8_t* state);

/* ---- GridBoxing: a second on-device game (18 actions, an adversary, signed rewards) ------ */

/* A small integer-only Boxing for n_envs simulators; ba3c_amd/boxing.py states the rules
 * (constants, step_numpy, render_numpy) and is the oracle of these entry points.  All game
 * state is int32, one 64-byte (16-byte aligned) row per simulator:
 *   game[e] = [ax, ay, ox, oy, a_cd, o_cd, a_score, o_score, t, rng, 0, 0, 0, 0, 0, 0]
 * (ax, ay) / (ox, oy): top-left of the agent's / the scripted opponent's 6x8 body (x in 4..74,
 * y in 14..70); a_cd / o_cd: steps until each may punch again (8 after a punch; the arm is
 * drawn while >= 6); a_score / o_score: points of the episode; t: its steps; rng: the
 * opponent LCG's uint32 bits; the six padding ints are written as 0.
 *
 * ba3c_boxing_step applies action[e] (ALE's 18: 0 NOOP, 1 FIRE, 2 UP, 3 RIGHT, 4 LEFT, 5 DOWN,
 * 6..9 the diagonals, 10..17 the same eight moves with FIRE; anything outside [0, 18) is
 * NOOP; the value is range-checked and shifts constant bit masks, it is never used as an
 * index) and writes reward[e] (float64: points landed minus points taken in this step),
 * over[e], and ep_score[e] ONLY where over[e] (a_score - o_score of the finished episode, in
 * [-101, 101]; the row is then already reset).  An episode ends when either score reaches
 * 100, at t >= 1680 (the clock) or at t >= limit (LimitLengthPlayer).  frame / state are as
 * for ba3c_breakout_step, and ba3c_boxing_render is ba3c_breakout_render for these rows.
 *
 * Same argument contract and host-side refusals as the Breakout pair, the same launch shape
 * (both games are one kernel template, one 256-thread workgroup per simulator). */
int ba3c_boxing_step(void* stream, int32_t* game, const int64_t* action, int32_t n_envs,
                     int32_t limit, double* reward, uint8_t* over, int32_t* ep_score,
                     uint8_t* frame, uint8_t* state);
int ba3c_boxing_render(void* stream, const int32_t* game, int32_t n_envs, uint8_t* frame,
                       uint8_t* state);

/* ---- Two-player GridBoxing: both boxers driven by actions (self-play, matches) ----------- */

/* A second way to run GridBoxing; ba3c_amd/duel.py states the rules (step_numpy, render_numpy,
 * mirror_rows) and is the oracle of these entry points.  The row is GridBoxing's,
 *   game[e] = [ax, ay, bx, by, a_cd, b_cd, a_score, b_score, t, rng, 0, 0, 0, 0, 0, 0]
 * with side B in the scripted opponent's fields; rng is carried unchanged (no draw is made).
 * n_games games have 2*n_games PLAYERS: player e is side A of game e, player n_games + e is
 * side B of game e, and action, reward, over, ep_score, frame and state all have 2*n_games rows
 * in that order.  Each side acts and sees in its own frame of reference, in which it is the
 * white boxer that starts on the left: side B's is the mirror x -> 78 - x of the world (its
 * RIGHT is the world's left, its dy is unchanged).
 *
 * ba3c_boxing_duel_step decodes both actions as ba3c_boxing_step does (ALE's 18, anything else
 * NOOP, never an index) and applies, in this order: both cooldowns count down; both boxers
 * move 2 px and are clamped; ONE judgement p in {0, 1, 2} of the reach on the positions after
 * both moves (GridBoxing's pts); a side that fires with its cooldown at 0 starts its cooldown
 * (8) and lands p; scores are added; a boxer that was hit is knocked 3 px away from the other
 * (side B to the right iff bx >= ax at the judgement) and clamped; t += 1.  reward[e] = points
 * landed by A minus points landed by B, reward[n_games + e] is its negative; over is shared
 * (either score >= 100, t >= 1680 or t >= limit); where over, ep_score[e] = a_score - b_score,
 * ep_score[n_games + e] its negative, and the row restarts as a fresh GridBoxing episode.
 * Side A's frame is ba3c_boxing_render's frame of the row, side B's that of the mirrored row
 * (78-bx, by, 78-ax, ay, b_cd, a_cd, b_score, a_score, t, rng); frame ([2G][84*84], may be
 * NULL) and state ([2G][84*84][4], may be NULL) are written as by ba3c_boxing_step, on over
 * both players' histories restart.
 *
 * ba3c_boxing_duel_render renders both sides of the current rows without stepping; with state
 * it starts both histories; with neither frame nor state it returns BA3C_OK without a launch.
 *
 * The host-side refusals are ba3c_boxing_step's / ba3c_boxing_render's (null game / action /
 * outputs, n_games < 1, limit < 1, misaligned game / state / frame -> BA3C_ERR_INVALID before
 * touching the device); they never synchronise and never allocate.  One launch, one 256-thread
 * workgroup per GAME, which steps the row once and renders both sides. */
int ba3c_boxing_duel_step(void* stream, int32_t* game, const int64_t* action, int32_t n_games,
                          int32_t limit, double* reward, uint8_t* over, int32_t* ep_score,
                          uint8_t* frame, uint8_t* state);
int ba3c_boxing_duel_render(void* stream, const int32_t* game, int32_t n_games, uint8_t* frame,
                            uint8_t* state);

/* One DECISION of every two-player game per call: frame skip and sticky actions per side, and
 * episodes that start from a drawn row.  ba3c_amd/duel.py (decide_numpy, "Drawn starts") states
 * the semantics and is the oracle.  aux[e] = [rng_k, rng_a, rng_b, prev_a, prev_b, 0, 0, 0]
 * (eight int32, 16-byte aligned rows): three LCG streams (the games' multiplier and increment),
 * one for the skip and one per side for its sticky draws, and each side's last effective action.
 * Per game, in this order:
 *   a, b = action[e], action[n_games + e], each 0 unless in [0, 32)
 *   rng_k = lcg(rng_k); k = skip_lo + (rng_k >> 16) % (skip_hi - skip_lo + 1)
 *   k times: rng_a = lcg(rng_a); prev_a = prev_a if ((rng_a >> 8) & 0xFFFF) < sticky_q16 else a;
 *            rng_b, prev_b likewise from b; one step of ba3c_boxing_duel_step's rules under
 *            (prev_a, prev_b); on over: prev_a = prev_b = 0, the remaining sub-steps are dropped
 * A fresh episode is GridBoxing's (20, 42, 58, 42) when start_lo == start_hi == 19, and draws
 * nothing; otherwise it is drawn from the ROW's rng, which no other rule touches:
 *   rng = lcg(rng); r = rng >> 16; h = start_lo + r % (start_hi - start_lo + 1);
 *   y = 14 + 2 * ((r >> 8) % 29); (ax, ay, bx, by) = (39 - h, y, 39 + h, y)
 * a row that is its own mirror image, so neither side is favoured.  reward[e] is the sum of side
 * A's rewards over the executed sub-steps and reward[n_games + e] its negative; over / ep_score
 * report the episode that ended; frame / state receive ONE frame per player, the one after the
 * last executed sub-step, as ba3c_boxing_duel_step writes them.  `limit` counts game steps.
 * With skip 1-1, sticky_q16 0 and start 19-19 a decision is exactly ba3c_boxing_duel_step.
 *
 * It refuses what ba3c_boxing_duel_step refuses, a null or not 16-byte aligned aux, a skip
 * outside 1 <= skip_lo <= skip_hi <= 16, a sticky_q16 outside [0, 65536] and a start outside
 * 4 <= start_lo <= start_hi <= 19, all on the host before touching the device; it never
 * synchronises and never allocates.  One launch, one 256-thread workgroup per game, the k steps
 * in registers. */
int ba3c_boxing_duel_decide(void* stream, int32_t* game, int32_t* aux, const int64_t* action,
                            int32_t n_games, int32_t limit, int32_t skip_lo, int32_t skip_hi,
                            int32_t sticky_q16, int32_t start_lo, int32_t start_hi, double* reward,
                            uint8_t* over, int32_t* ep_score, uint8_t* frame, uint8_t* state);

/* ---- Frame skip and sticky actions for the on-device games ------------------------------- */

/* One DECISION per call instead of one game step: ALE's `-v0` behaviour of a frame skip drawn
 * per decision and of sticky actions.  ba3c_amd/frameskip.py states the semantics and is the
 * oracle.  aux[e] = [rng2, prev] (two int32, 8-byte aligned rows) is the decision's own LCG
 * (the games' multiplier and increment; a stream separate from the row's rng) and the last
 * effective action.  Per simulator, in this order:
 *   a = action[e] if 0 <= action[e] < 32 else 0
 *   rng2 = lcg(rng2); k = skip_lo + (rng2 >> 16) % (skip_hi - skip_lo + 1)
 *   k times: rng2 = lcg(rng2); eff = prev if ((rng2 >> 8) & 0xFFFF) < sticky_q16 else a;
 *            prev = eff; one game step under eff (the rules of ba3c_*_step, unchanged);
 *            on over: prev = 0 and the remaining sub-steps are dropped
 * reward[e] is the sum over the executed sub-steps, over[e] / ep_score[e] report the episode
 * that ended, frame / state receive ONE frame, the one after the last executed sub-step (on
 * over: the new episode's first, the history cleared), as ba3c_*_step writes them.  `limit`
 * counts game steps (the row's t), not decisions.
 *
 * They refuse what ba3c_*_step refuses and a null or misaligned aux, a skip outside
 * 1 <= skip_lo <= skip_hi <= 16 and a sticky_q16 outside [0, 65536] (65536: every sub-step
 * repeats prev), all on the host before touching the device.  One launch, one 256-thread
 * workgroup per simulator, the k steps in registers. */
int ba3c_breakout_step_skip(void* stream, int32_t* game, int32_t* aux, const int64_t* action,
                            int32_t n_envs, int32_t limit, int32_t skip_lo, int32_t skip_hi,
                            int32_t sticky_q16, double* reward, uint8_t* over, int32_t* ep_score,
                            uint8_t* frame, uint8_t* state);
int ba3c_boxing_step_skip(void* stream, int32_t* game, int32_t* aux, const int64_t* action,
                          int32_t n_envs, int32_t limit, int32_t skip_lo, int32_t skip_hi,
                          int32_t sticky_q16, double* reward, uint8_t* over, int32_t* ep_score,
                          uint8_t* frame, uint8_t* state);

/* ---- The colour view of the on-device games ---------------------------------------------- */

/* Draw the CURRENT game of selected simulators as RGB images; ba3c_amd/view.py (view_numpy)
 * states the image and is the oracle.  Image i shows simulator sel[i] (sel null: simulator i;
 * n_sel images either way); an index outside [0, n_envs) gives an all-zero image.  The canvas is
 * 84 px wide and Hc = 84 high, or Hc = 104 with hud: rows 0..83 are palette[shade] of the frame
 * ba3c_*_render draws (palette: 256 RGB triples), rows 84..103 the HUD strip of view.py drawn
 * from hud[i] (20 bytes: the bar heights of actions 0..17, the chosen action or 255, the value
 * bar's length; the kernel clamps them).  Canvas pixel (y, x) fills the scale x scale block at
 * (y*scale, x*scale) of out = uint8 [n_sel][Hc*scale][84*scale][3].
 *
 * The launch reads game, sel, hud and palette and writes out only: no game row, aux row or
 * history is written.  They refuse a null game / palette / out, n_envs < 1, n_sel < 1, a scale
 * outside [1, 8], a game that is not 16-byte and a sel / hud / out that is not 4-byte aligned,
 * all on the host before touching the device.  One launch, one 256-thread workgroup per image. */
int ba3c_breakout_view(void* stream, const int32_t* game, int32_t n_envs, const int32_t* sel,
                       int32_t n_sel, const uint8_t* palette, const uint8_t* hud, int32_t scale,
                       uint8_t* out);
int ba3c_boxing_view(void* stream, const int32_t* game, int32_t n_envs, const int32_t* sel,
                     int32_t n_sel, const uint8_t* palette, const uint8_t* hud, int32_t scale,
                     uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* BA3C_H */
