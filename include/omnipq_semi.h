/* omnipq_semi.h -- C ABI of the semi-supervised criteria: the gamma-mixture guide.
 *
 * Reference: models/utils/gamma_mixture_loss_util.py:130-191 `gamma_mixture_guide_criterion(end_points, DATASET_CONFIG,
 * config)` and :27-127 `quad_point_mixture_metric`, called by train.py:513 on the unlabelled half of the batch.  Per scene
 * the reference picks one quad whose score passes 0.1 (`random.choice`), samples K = 10 000 points with replacement
 * (`torch.randint`), measures a distance of every sample to the quad, labels the samples with fit.py:152-174 `fit_gamma`
 * and turns the kept ones into four metrics -- about sixty small PyTorch ops, several `.item()` reads and a numpy round
 * trip per scene.
 *
 * `fit_gamma` runs 25 EM steps and then labels with the two distributions it built from its ARGUMENTS (fit.py:160,
 * :168-173), which the fit never touches.  With the call site's arguments (:65: a1 = 2, b1 = 20, a2 = 3, b2 = 1,
 * weight = 0.1) a sample of distance t is kept iff
 *     0.1 * (20^2 / Gamma(2)) * e^(-20 |t|) * |t|  >=  0.9 * (1 / Gamma(3)) * e^(-|t|) * |t|^2
 * i.e. |t| <= t* = 0.29961316955346434; t = 0 is kept, NaN is not.  The criterion is therefore a fixed function of its
 * inputs and of the two draws, and runs here without a host read: three launches forward (draw, one workgroup per scene,
 * a one-wave reduction over the scenes in scene order), one backward.  Sums accumulate in f64 in a fixed order and the
 * order statistics come from an integer radix selection: the same inputs and draws give the same bits.
 *
 * Conventions as in omnipq_pointops.h: device pointers, sizes, a hipStream_t, int return (0 = ok); arguments are
 * validated before the device is touched (OMNIPQ_EINVAL: b < 0, k < 1, n < 1, q < 1, xyz_pitch < 3, a null required
 * pointer; OMNIPQ_ETOOLARGE: k > OMNIPQ_GM_MAX_K); b == 0 succeeds and does nothing.
 */
#ifndef OMNIPQ_SEMI_H
#define OMNIPQ_SEMI_H
#ifdef __cplusplus
extern "C" {
#endif

/* The kept samples' distances of one scene are selected from in the workgroup's LDS, 4 bytes per sample: 60 KiB. */
#define OMNIPQ_GM_MAX_K 15360
/* floats per scene of the record the forward leaves for the backward:
 *   [0..3] the scene's metric_normal, metric_vertical, metric_size, metric_score (0 when the scene does not count)
 *   [4] 1 if the scene counts (a candidate quad, pick in range, n_k >= 300), else 0      [5] n_k
 *   [6] q85 of the kept vertical distances      [7..9] mean of the kept points      [10] pseudo_x
 *   [11] score branch: 0 none, 1 CE(score, 1), 2 CE(score, 0) */
#define OMNIPQ_GM_RECORD_FLOATS 12

/* The two draws of :149-177.  quad_scores (b, q, 2) f32.  Candidates of scene s: {j : softmax(quad_scores[s, j])[1] > 0.1}.
 * skip[s] = 1 and pick[s] = 0 when there are none; else skip[s] = 0 and pick[s] = the r-th candidate in index order, r
 * uniform over their number.  sample_inds (b, k) int32: uniform in [0, n), with replacement.  Randomness: a counter hash
 * of (*seed -- 64 bits in DEVICE memory, read by the kernel --, salt, scene, i), as the dropout of the decoder kernels
 * (pointnet2/dropout_state.py): a captured launch draws afresh on every replay that finds the counter advanced, and the
 * same counter value gives the same draws. */
int omnipq_gm_draw(int b, int n, int q, int k, const float *quad_scores, const unsigned long long *seed, unsigned salt,
                   int *pick, int *skip, int *sample_inds, void *stream);

/* quad_point_mixture_metric (:27-127) of the picked quad of every scene, and the sum over the scenes / b (:185-192; a
 * skipped scene counts in b).
 *   xyz (b, n, xyz_pitch) f32, only columns 0..2 are read; normals (b, n, 3); quad_scores (b, q, 2); quad_center (b, q, 3);
 *   normal_vector (b, q, 3); quad_size (b, q, 2); pick (b) int32; skip (b) int32 or NULL (NULL: derived from quad_scores as
 *   omnipq_gm_draw does); sample_inds (b, k) int32.
 * A pick outside [0, q) skips the scene; a sample index outside [0, n) is never read and counts as dropped.
 * With c, nv, s, score of the picked quad:  s0 = s[0] / 1.5 (NOT written back: the reference divides the caller's tensor
 * in place, :29), s1 = s[1], n = (nv.x, nv.y, 0) / |(nv.x, nv.y)|, xdir = (-n.y, n.x, 0); per sample x with normal m:
 *   mh = m / max(|m|, 1e-5), dc = 1 - |n . mh|, o = x - c, v = |o . n|, xd = |o . xdir|, zd = |o.z|,
 *   A = |max(2 (xd, zd) - (s0, s1), 0)|, total = 2.5 dc + 0.2 A^2 + 0.5 v     (f32; `size_distance_B`, :57, is unused)
 *   keep: the inequality above on (double)total.
 * n_k = number kept; n_k < 300 (:78) or a skipped scene: the four terms are 0.  Otherwise
 *   metric_normal   = 1 - |cos(est, n)|, est = normalise((mean_keep(m).x, mean_keep(m).y, 0)), eps 1e-8
 *   metric_vertical = sum_keep v [v < q85] / n_k, q85 = quantile(v_keep, 0.85)
 *   metric_size     = sl1(s0 - 2 pseudo_x) + sum_3 sl1(mu - c), mu = mean_keep(x), xd' = |(x - mu) . xdir| over the kept,
 *                     pseudo_x = mean over t in {0.85, 0.925, 1} of quantile(xd', t) / t, sl1 = models/utils/losses.py:5-13
 *                     with delta 1.  The z candidate (:110, :115) carries the weight `0.` in the reference and is NOT
 *                     computed here.
 *   metric_score    = CE(score, 1) if mv < 0.05 and mn < 0.02 and ms < 0.10; CE(score, 0) if mv > 0.3 or mn > 0.05 or
 *                     ms > 0.35; else 0
 * quantile = torch.quantile's default: rank = t (n_k - 1) in f32, lerp between the two bracketing order statistics.
 * record: float[b][OMNIPQ_GM_RECORD_FLOATS]; terms: float[4]; both overwritten. */
int omnipq_gm_guide(int b, int n, int q, int k, int xyz_pitch, const float *xyz, const float *normals,
                    const float *quad_scores, const float *quad_center, const float *normal_vector, const float *quad_size,
                    const int *pick, const int *skip, const int *sample_inds, float *record, float *terms, void *stream);

/* Backward in one launch: g_terms float[4] = dLoss/dterms -> g_quad_scores (b, q, 2), g_quad_center (b, q, 3), g_quad_size
 * (b, q, 2), all overwritten, zero outside the picked rows:
 *   d mv / d c = -sum_keep [v < q85] sign(o . n) n / n_k;   d ms / d c = -sl1'(mu - c);   d ms / d s[0] = sl1'(s0 - 2 pseudo_x) / 1.5
 *   the cross-entropy gradient of the recorded branch to the two scores; everything divided by b.
 * Nothing flows to normal_vector, to quad_size[..., 1] or through metric_normal: the reference detaches them (`.detach()`
 * :35/:47, `.item()` :89, `torch.tensor([...])` :114, the numpy round trip :65). */
int omnipq_gm_guide_grad(int b, int n, int q, int k, int xyz_pitch, const float *xyz, const float *normals,
                         const float *quad_scores, const float *quad_center, const float *normal_vector,
                         const float *quad_size, const int *pick, const int *sample_inds, const float *record,
                         const float *g_terms, float *g_quad_scores, float *g_quad_center, float *g_quad_size, void *stream);

#ifdef __cplusplus
}
#endif
#endif
