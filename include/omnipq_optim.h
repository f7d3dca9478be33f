/*
 * omnipq_optim.h -- C ABI of the fused gradient clipping + AdamW step (libomnipq_pointops.so).
 *
 * The three lines of the reference's training step that change the weights (train.py:562-566)
 *     grad_total_norm = clip_grad_norm_(model.parameters(), config.clip_norm)
 *     optimizer.step()          AdamW over two parameter groups, train.py:364-374
 * as three launches over ALL parameter tensors: squared-norm partials, finalise, update.  No launch takes a
 * hyper-parameter as a kernel argument: learning rates, betas, eps, weight decay, max_norm and grad_scale are read from
 * device memory, and so are the step count and the bias corrections -- a launch captured into a hipGraph follows a
 * learning-rate schedule when it is replayed.
 *
 * Device data (all pointers below are device pointers unless a name ends in _host):
 *   records   nrec packed 48-byte records
 *                 { float *param; const float *grad; float *exp_avg; float *exp_avg_sq; int64_t numel; int32_t group;
 *                   int32_t reserved; }
 *             contiguous f32 tensors at ANY 4-byte-aligned address (parameters may be views into joint matrices): a chunk whose
 *             tensors share one phase modulo 16 bytes moves as 16-byte vectors around a peeled head and tail, any other chunk
 *             element by element.
 *   chunks    nchunks x int32[2] = { record, chunk of `chunk_elems` elements of it }; chunk_elems is a multiple of 1024.
 *   hyper     (ngroups + 1) rows of 8 doubles.  Row g < ngroups: { lr, beta1, beta2, eps, weight_decay, 0, 0, 0 } of
 *             parameter group g; row ngroups: { max_norm, grad_scale, ema_decay, 0, ... } (ema_decay is read
 *             by omnipq_adamw_ema_finalize only).  Doubles, because torch.optim.AdamW
 *             evaluates 1 - beta2, 1 - lr * weight_decay, lr / (1 - beta1^t) and sqrt(1 - beta2^t) in double precision
 *             before it rounds them to the tensors' f32.
 *   partials  nchunks doubles (scratch).
 *   counters  int64[2] = { t, skipped }: optimiser steps taken, steps skipped for a non-finite gradient norm.
 *   result    float[4] = { total_norm, clip_coef, found_nonfinite (0 or 1), grad_scale * clip_coef }.
 *   coef      ngroups rows of 8 floats, written by the finalise launch for the update launch:
 *             { 1 - lr * wd, beta1, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), eps }.
 *
 * Gradient accumulation (the reference's step_freq: train.py:493-494 zeroes the gradients on the first of k micro-batches only,
 * train.py:562-576 clips, steps and averages on the last; the loss is not divided, so the gradients are SUMMED) is the
 * omnipq_adamw_accum_* family: the same three launches on EVERY micro-batch, so that one captured graph serves all of them.
 *   acc       a flat f32 accumulator laid out exactly like the flat exp_avg buffer the records point into: the segment of a
 *             record is acc_base + (rec.exp_avg - exp_avg_base), so p, m, v and acc of a chunk share one phase modulo 16 bytes.
 *             The two bases are fixed addresses passed as arguments; the record layout is unchanged.
 *   accum     int64[2] = { micro, apply }: micro-batches already summed, in [0, accum_steps), and whether the last finalise
 *             launch was the applying one (0 or 1).  Written by the finalise launch only, with ordinary stores of thread 0.
 *   accum_steps (k) is a kernel argument: it is fixed for the life of a captured launch.
 * On an applying call result[0..3] mean what they mean above; on any other call only result[0] (the norm of grad_scale times
 * the running sum) is written.  The sum is overwritten, not added to, when micro == 0: no zeroing launch, and a non-finite value
 * left behind by a skipped step cannot leak into the next one.
 *
 * Mean-teacher weight averaging (the reference's update_ema_variables, train.py:435-439, called after optimizer.step() at
 * train.py:576) inside the same launches is the omnipq_adamw_ema_* pair; the squared-norm launch is the one above, unchanged.
 *     alpha = min(1 - 1 / (global_step + 1), decay);   ema = alpha * ema + (1 - alpha) * param
 * alpha changes with every step, so it cannot be a kernel argument of a captured launch: the finalise launch forms it from a
 * device word and the update launch reads it, like the bias corrections.
 *   hyper     row ngroups, slot 2: ema_decay (a double like the rest of the row).
 *   ema_state int64[1]: the global_step the NEXT averaging will use.  Written by thread 0 of the finalise launch only, with an
 *             ordinary store.
 *   ema_coef  float[2] = { alpha, beta }, written by the finalise launch for the update launch.  In f64:
 *             a = fmin(1 - 1 / (double)(global_step + 1), decay); alpha = (float)a, beta = (float)(1 - a) -- the two roundings
 *             the float arguments of omnipq_ema_update (omnipq_sa.h) go through when Python doubles reach them.
 *   ema_ptrs  nrec device pointers: entry i is the teacher's tensor paired with records[i].param (contiguous f32 of the same
 *             numel, 4-byte aligned).  A parallel array: the 48-byte record does not change.
 *   ema_only  n_only packed 24-byte records { float *ema; const float *param; int64_t numel; } (the segment layout of
 *             omnipq_ema_update) with only_chunks, n_only_chunks x int32[2] = { record, chunk of `chunk_elems` elements of it }:
 *             the pairs whose student parameter is not in `records` because it has no gradient.  The reference averages every
 *             parameter, whether or not it received a gradient.
 * An APPLYING call is every call of the plain family and the accum_steps-th micro-batch of the accumulating one.  It always
 * averages: a step skipped for a non-finite gradient norm leaves p, m and v alone and still averages the teacher with the
 * unchanged p, as a training loop on the separate call does (train.py:576 does not look at the norm).  Any other micro-batch
 * touches neither the teacher nor ema_state.  Per element: t = ema * alpha rounded to f32, then ema = fmaf(beta, p_new, t) --
 * the arithmetic of omnipq_ema_update, so the teacher holds the same bits as after that call on the updated parameters.
 *
 * Dynamic fp16 loss scaling (the two tensors and the recurrence of torch.amp.GradScaler: torch._amp_update_scale_) is one more
 * scalar recurrence in the finalise launch: omnipq_adamw_scaled_finalize, the superset of the three finalise entry points above.
 * The squared-norm and update launches are the ones above, unchanged; they see the scale only through result[3].
 *   scaler_state  one struct omnipq_loss_scaler { scale, growth_tracker } in device memory: GradScaler's `_scale` and
 *                 `_growth_tracker`; omnipq_loss_scaler_record() reports its layout to a binding.  The caller multiplies its loss by `scale` (a device read: nothing of it is a kernel argument), so the gradients
 *                 arrive as S * g.  Written by thread 0 of the finalise launch only, with ordinary stores.
 *   scaler_cfg    double[4] = { growth_factor, backoff_factor, growth_interval, 0 } in device memory: a changed interval, like a
 *                 loaded scale, takes effect on the next replay of the same captured launch.
 * With S = scaler_state->scale read at entry and inv = 1 / (double)S:
 *     total_norm = (float)(sqrt(sum of partials) * inv)            the norm of the UNSCALED gradients (times grad_scale)
 *     result[3]  = (float)(grad_scale * inv) * clip_coef           the effective factor is grad_scale / S
 * A micro-batch that is not the applying one touches neither scale nor growth_tracker, so S is constant over an accumulation
 * window -- which the sum of scaled gradients requires.  An applying call then runs, after everything the other finalise entry
 * points do:
 *     norm not finite:  scale = (float)((double)scale * backoff_factor);  growth_tracker = 0
 *     norm finite:      growth_tracker += 1;  when it equals growth_interval: the candidate (float)((double)scale * growth_factor)
 *                       replaces scale only if it is finite, and growth_tracker = 0 either way.
 * The detector is the NORM, as it already is for `skipped`, not torch's per-tensor found_inf: the two differ only when finite
 * gradients have a norm that overflows f32.  result[3] is ONE f32 for un-scaling and clipping together, where torch multiplies
 * twice: where grad_scale * clip_coef / S falls below 2^-126 (S beyond 2^120 or so) it is a subnormal f32 and holds fewer than
 * 24 bits unless it is a power of two.  S = 0 (after ~150 back-offs in a row) makes every later norm non-finite, as in torch.
 *
 * `.grad` is READ-ONLY here: the clipped (and un-scaled) gradient g' = grad_scale * clip_coef * g exists in registers
 * only and is never written back.  Nothing in the reference reads the gradients after train.py:564; a caller that wants the
 * clipped gradients in memory must keep torch.nn.utils.clip_grad_norm_.
 *
 * Every entry point validates its host arguments (null tables or bases, negative counts, ngroups < 1, accum_steps < 1, a chunk
 * size that is not a positive multiple of 1024) and returns OMNIPQ_EINVAL before anything is launched.  What a DEVICE table holds cannot be seen
 * from the host: omnipq_adamw_check_table validates the host copy a binding is about to upload.
 */
#ifndef OMNIPQ_OPTIM_H
#define OMNIPQ_OPTIM_H
#ifdef __cplusplus
extern "C" {
#endif

/* HOST arrays, nothing is launched: OMNIPQ_EINVAL for a record with a null pointer, a negative numel or a `group` outside
 * [0, ngroups), and for a chunk entry that names no record or lies past its record's last element. */
int omnipq_adamw_check_table(int nrec, const void *records_host, int nchunks, const int *chunks_host, int ngroups,
                             int chunk_elems);

/* clip_grad_norm_, first half (train.py:562; torch/nn/utils/clip_grad.py: the 2-norm over all gradients):
 * partials[c] = sum over chunk c of (grad_scale * g)^2, accumulated in f64 in a fixed order.  No atomics: the same
 * gradients give the same bits. */
int omnipq_adamw_grad_sqnorm(int nrec, int nchunks, const void *records, const int *chunks, int chunk_elems,
                             const double *hyper, int ngroups, double *partials, void *stream);

/* clip_grad_norm_, second half, and the scalar part of AdamW.step (train.py:562-563), one workgroup:
 *   total_norm = sqrt(sum of partials)  (f64, rounded once to f32)    clip_coef = min(1, max_norm / (total_norm + 1e-6)),
 *   1 when max_norm <= 0;  found_nonfinite = !isfinite(total_norm).  Finite: t += 1 and the bias corrections 1 - beta^t in
 *   f64 -> coef.  Otherwise skipped += 1 (the skip rule of torch.amp.GradScaler.step). */
int omnipq_adamw_finalize(int nchunks, const double *partials, const double *hyper, int ngroups, long long *counters,
                          float *result, float *coef, void *stream);

/* AdamW.step (train.py:563; torch/optim/adamw.py) over all chunks with g' = grad_scale * clip_coef * g:
 *   p *= 1 - lr * wd;  m = beta1 * m + (1 - beta1) * g';  v = beta2 * v + (1 - beta2) * g'^2;
 *   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps).
 * A no-op for every element when result[2] (found_nonfinite) is set. */
int omnipq_adamw_update(int nrec, int nchunks, const void *records, const int *chunks, int chunk_elems,
                        const float *coef, const float *result, void *stream);

/* Accumulate + squared norm: a = (micro == 0) ? g : acc + g (one f32 add), acc = a, and
 * partials[c] = sum over chunk c of (grad_scale * a)^2 in f64, in the order of omnipq_adamw_grad_sqnorm on a gradient at the
 * same address -- the same bits as that call on the summed gradients.  The gradient is read once; no atomics. */
int omnipq_adamw_accum_sqnorm(int nrec, int nchunks, const void *records, const int *chunks, int chunk_elems,
                              const double *hyper, int ngroups, const float *exp_avg_base, float *acc_base,
                              const long long *accum, double *partials, void *stream);

/* Finalise of one micro-batch, one workgroup.  result[0] = grad_scale * |running sum| always.  micro != accum_steps - 1:
 * micro += 1, apply = 0, nothing else is touched.  micro == accum_steps - 1: everything omnipq_adamw_finalize does (clip
 * coefficient; non-finite: skipped += 1; else t += 1 and the coef rows), then micro = 0 and apply = 1. */
int omnipq_adamw_accum_finalize(int nchunks, const double *partials, const double *hyper, int ngroups, int accum_steps,
                                long long *counters, long long *accum, float *result, float *coef, void *stream);

/* omnipq_adamw_update with the gradient read from the record's accumulator segment.  A no-op for every element when apply is 0
 * or result[2] (found_nonfinite) is set. */
int omnipq_adamw_accum_update(int nrec, int nchunks, const void *records, const int *chunks, int chunk_elems,
                              const float *exp_avg_base, const float *acc_base, const long long *accum, const float *coef,
                              const float *result, void *stream);

/* HOST arrays, nothing is launched: OMNIPQ_EINVAL for a null or misaligned teacher pointer among the nrec entries of
 * ema_ptrs_host, for an ema_only record with a null or misaligned pointer or a negative numel, and for an only_chunks entry that
 * names no record or lies past its record's last element. */
int omnipq_adamw_check_ema_table(int nrec, const void *ema_ptrs_host, int n_only, const void *ema_only_host,
                                 int n_only_chunks, const int *only_chunks_host, int chunk_elems);

/* omnipq_adamw_finalize (accum == NULL; accum_steps must then be 1) or omnipq_adamw_accum_finalize (accum != NULL) plus, on
 * an applying call and whether or not the norm is finite: g = ema_state[0], ema_coef = { alpha, beta } of global_step g and
 * the decay in hyper, ema_state[0] = g + 1.  A micro-batch that is not the applying one touches neither. */
int omnipq_adamw_ema_finalize(int nchunks, const double *partials, const double *hyper, int ngroups, int accum_steps,
                              long long *counters, long long *accum, long long *ema_state, float *result, float *coef,
                              float *ema_coef, void *stream);

/* omnipq_adamw_update (accum == NULL) or omnipq_adamw_accum_update (accum != NULL: exp_avg_base and acc_base are then
 * required) over nchunks workgroups, each of which also averages the teacher's copy of its chunk with the p it has just
 * computed, plus n_only_chunks workgroups that average the chunks of ema_only with p as it is in memory.  The teacher's chunk
 * moves as 16-byte vectors where it shares p's phase modulo 16 bytes (a deep copy does) and through 4-byte-aligned accesses
 * where it does not.  apply == 0: a no-op.  result[2] (found_nonfinite) set: p, m and v stay, every workgroup averages. */
int omnipq_adamw_ema_update(int nrec, int nchunks, const void *records, const void *ema_ptrs, const int *chunks,
                            int chunk_elems, int n_only, int n_only_chunks, const void *ema_only, const int *only_chunks,
                            const float *exp_avg_base, const float *acc_base, const long long *accum, const float *coef,
                            const float *ema_coef, const float *result, void *stream);

/* The dynamic loss scale in device memory: torch.amp.GradScaler's two tensors (`_scale` f32, `_growth_tracker` int32). */
struct omnipq_loss_scaler {
  float scale;          /* S: the loss is multiplied by it, the gradients arrive scaled by it */
  int growth_tracker;   /* applying calls with a finite norm since the scale last changed (32 bits) */
};

/* The layout of struct omnipq_loss_scaler as THIS build compiled it, one line in the format of omnipq_abi_records()
 * (omnipq_pointops.h): "struct omnipq_loss_scaler scale:f growth_tracker:i".  A binding builds the device struct from this
 * text; the library asserts at compile time that the text states the sizes and offsets the compiler uses. */
const char *omnipq_loss_scaler_record(void);

/* The superset finalise, one workgroup: omnipq_adamw_finalize (accum == NULL; accum_steps must then be 1) or
 * omnipq_adamw_accum_finalize (accum != NULL), with the teacher's coefficients of omnipq_adamw_ema_finalize when ema_state and
 * ema_coef are set (both NULL or both set), the norm and result[3] divided by scaler_state->scale, and on an applying call the
 * recurrence of torch._amp_update_scale_ on scaler_state with the factors of scaler_cfg (see the head of this file).
 * OMNIPQ_EINVAL, before anything is launched: a null scaler_cfg or scaler_state, only one of ema_state / ema_coef, accum ==
 * NULL with accum_steps != 1, and everything the other finalise entry points refuse. */
int omnipq_adamw_scaled_finalize(int nchunks, const double *partials, const double *hyper, int ngroups, int accum_steps,
                                 long long *counters, long long *accum, long long *ema_state, float *ema_coef,
                                 const double *scaler_cfg, struct omnipq_loss_scaler *scaler_state, float *result,
                                 float *coef, void *stream);

/* The learning-rate schedule of the reference's utils/lr_scheduler.py: get_scheduler (GradualWarmupScheduler in front of
 * CosineAnnealingLR or MultiStepLR, train.py:566 `scheduler.step()`) as one more scalar recurrence of the finalise launch.
 * With e = sched_state[0], the number of scheduler.step() calls so far, W = warmup_iters and b = base_lr[g], in f64 and in this
 * operation order (tests/lr_schedule_restatement.py is the same text in Python):
 *     W > 0 and e <= W:   b / multiplier * ((multiplier - 1.) * e / W + 1.)          (at e == W this is not b for every b)
 *     otherwise, k = e - W (k = e when W <= 0):
 *       kind 0 (cosine):  eta_min + (b - eta_min) * (1 + cos(pi * k / t_max)) / 2
 *       kind 1 (step):    b * gamma_pow[j],  j = the number of milestones <= k (bisect_right over the sorted milestones)
 * gamma_pow[j] = gamma ** j is filled by the host, so the device needs no pow and the step schedule keeps the host's bits.
 * The struct lives in DEVICE memory: a field changed there is seen by the next replay of a captured launch.  What a device
 * struct holds cannot be checked from the host; a binding validates its host copy (kind 0 or 1, t_max >= 1, multiplier > 1,
 * warmup_iters >= 0, 0 <= n_milestones <= omnipq_lr_schedule_max_milestones(), milestones sorted). */
struct omnipq_lr_schedule {
  int kind;                 /* 0 = cosine annealing, 1 = multi-step */
  int n_milestones;         /* entries of `milestones` in use (kind 1) */
  long long warmup_iters;   /* W; 0 = no warm-up */
  long long t_max;          /* CosineAnnealingLR's T_max, in scheduler steps behind the warm-up */
  double multiplier;        /* GradualWarmupScheduler's multiplier: the warm-up starts at b / multiplier */
  double eta_min;           /* CosineAnnealingLR's eta_min */
  long long milestones[8];  /* sorted, in scheduler steps behind the warm-up; duplicates count once each */
  double gamma_pow[9];      /* gamma ** j for j = 0 .. 8 */
};

/* The layout of struct omnipq_lr_schedule as THIS build compiled it, one line in the format of omnipq_abi_records(), and the
 * length of its `milestones` array.  The text and the static_asserts that hold it to the compiler's layout are written by
 * omni-pq_amd/build.py from the definition above. */
const char *omnipq_lr_schedule_record(void);
int omnipq_lr_schedule_max_milestones(void);

/* lr_now[g] = the schedule's value for e = sched_state[0] and base_lr[g], g < ngroups: one small launch.  For attach time and
 * after a loaded state, so that lr_now always holds the device's own bits.  OMNIPQ_EINVAL, before anything is launched:
 * ngroups < 1 or a null pointer. */
int omnipq_lr_schedule_eval(int ngroups, const struct omnipq_lr_schedule *sched, const double *base_lr,
                            const long long *sched_state, double *lr_now, void *stream);

/* The superset of omnipq_adamw_scaled_finalize, one workgroup, the same kernel body: loss scaler (scaler_cfg and scaler_state:
 * both NULL or both set), teacher (ema_state and ema_coef: both or neither), accumulation (accum) and schedule (sched, base_lr,
 * sched_state and lr_now: all four or none) are each optional.  With a schedule the coefficient rows are formed with lr_now[g]
 * in place of hyper[g][0]; then, on every APPLYING call and whether or not the norm is finite (train.py:566 does not look at
 * the norm), sched_state[0] += 1 and lr_now is re-evaluated -- the value param_groups shows after scheduler.step().  A
 * micro-batch that is not the applying one touches neither.  Thread 0 does all of it with ordinary stores.
 * OMNIPQ_EINVAL, before anything is launched: an incomplete pair or quadruple, accum == NULL with accum_steps != 1, and
 * everything the other finalise entry points refuse. */
int omnipq_adamw_sched_finalize(int nchunks, const double *partials, const double *hyper, int ngroups, int accum_steps,
                                long long *counters, long long *accum, long long *ema_state, float *ema_coef,
                                const double *scaler_cfg, struct omnipq_loss_scaler *scaler_state,
                                const struct omnipq_lr_schedule *sched, const double *base_lr, long long *sched_state,
                                double *lr_now, float *result, float *coef, void *stream);

/* Windowed statistics of the step's reported scalars (the reference's stat_dict loop, train.py:580-586: `stat_dict[key] +=
 * end_points[key].item()` on the applying micro-batch), without a host read: one thread per entry, a grid of ceil(n / 256)
 * workgroups, no atomics, capturable.
 *   entries  n packed 16-byte records { const void *src; int32 kind (0 = f32, 1 = f64); int32 mode (0 = sum, 1 = last value) }
 *            in device memory; src points at one device scalar.
 *   sums     n doubles: mode 0: sums[i] += (double)*src -- the sequential f64 sum in call order, the bits of the reference's
 *            Python-float `+=`; NaN and Inf propagate as there.  mode 1: sums[i] = (double)*src.
 *   last     n doubles: last[i] = (double)*src, whatever the mode.
 *   window   int64[2] = { steps accumulated, calls seen }, written by thread 0 of workgroup 0.
 *   accum    the optimiser's { micro, apply } word or NULL.  Non-NULL with apply == 0: the call only increments `calls seen`.
 * OMNIPQ_EINVAL, before anything is launched: n outside [1, 4096] or a null entries, sums, last or window. */
int omnipq_stats_accumulate(int n, const void *entries, double *sums, double *last, long long *window,
                            const long long *accum, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OMNIPQ_OPTIM_H */
