/* omnipq_semi.h -- C ABI of the semi-supervised criteria: the gamma-mixture guide and, below it, the mean-teacher
 * consistency loss and the ARKit physical-constraint loss.
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

/* ---- mean-teacher consistency loss -------------------------------------------------------------------------------------
 * Reference: models/utils/mean_teacher_consistency_util.py:201-270 `get_consistency_loss(end_points, ema_end_points,
 * DATASET_CONFIG)`, called by train.py:531 with the student's and the teacher's outputs.  For each of `prefixes` prediction
 * heads and each of two kinds (0 objects, 1 quads; "pk" = 2 * prefix + kind below), per scene s with k proposals:
 *
 *   align    e = teacher centre; x negated where flip_x[s] != 0, y where flip_y[s] != 0; e <- e rot_mat[s]^T; e <- e scale[s].
 *            NOT written back to the teacher's tensor (the reference flips it in place, :32-35): e goes to `ema_center`.
 *   assign   ind1[i] = argmin_j |c_i - e_j|^2, dist1[i] the minimum; ind2[j] = argmin_i |c_i - e_j|^2, dist2[j] (c: the
 *            student's centres; first index on ties);  conf[r] = softmax(score[s, r])[1] of the STUDENT (objectness_scores /
 *            quad_scores);  d[r] = dist1[r] conf[ind1[r]] + dist2[r] conf[r]   (ind1 indexes the student's scores: :45)
 *   clip     eps = torch.quantile(v, 0.85) over all b * k values v of the call (rank in f32, lerp between the bracketing order
 *            statistics); term = sum_r [v_r < eps] v_r / (b k); no gradient through eps.  Applied to d and to the three
 *            distances below.
 *   objects  a = ind2.  class = 2 * sum_{r,c} pT[r,c] (log pT[r,c] - log pS[a_r,c]) / (b k nc), p = softmax(sem_cls_scores);
 *            size(x) = mean_size[argmax size_scores] + size_residuals[argmax], the teacher's times scale[s];
 *            dsz[r] = |size_S[a_r] - size_T[r]|^2 conf[r], clipped.
 *   quads    dn[r] = (1 - |cos(nS[a_r].xy, nT[r].xy)|) conf[r] (cos as torch's cosine_similarity: each vector divided by
 *            max(|.|, 1e-8); the teacher's normal is NOT aligned, as in the reference), clipped;
 *            dqs[r] = |quad_size_S[a_r] - quad_size_T[r]|^2 conf[r], clipped;
 *            qclass = 2 * sum_{r,c} KL as above over quad_scores / b  (`batchmean`; weight 0 in the total, still reported).
 *   per prefix   obj = 0.5 centre + class + 0.05 size;   quad = 0.5 centre_q + 0 qclass + normal + 0.05 size_q
 *   terms[0..8]  the sums over the prefixes / prefixes of: centre, class, size, obj, centre_q, qclass, normal, size_q, quad
 *   terms[9]     terms[3] + terms[8]
 *
 * Everything per row is computed in f64 from the f32 inputs; the clipped values are stored as f32 and selected from by the
 * integer radix selection of the guide; sums are f64 in a fixed order: the same inputs give the same bits.  No float atomics,
 * no host read.  Forward: three launches (rows: grid (b, 2 prefixes); clip: one workgroup per pk; a one-wave fold in prefix
 * order).  Backward: one launch, grid (b, 2 prefixes); every gradient row is written exactly once (a gather over the stored
 * assignments and masks), nothing is accumulated into.
 *
 * OMNIPQ_EINVAL: a null required pointer, b < 0, k < 1, prefixes outside [1, OMNIPQ_MT_MAX_PREFIXES], nc or ns outside
 * [1, OMNIPQ_MT_MAX_CLASSES].  OMNIPQ_ETOOLARGE: k > OMNIPQ_MT_MAX_K or b * k > OMNIPQ_MT_MAX_ROWS.  b == 0 succeeds and does
 * nothing. */
#define OMNIPQ_MT_MAX_PREFIXES 8
#define OMNIPQ_MT_MAX_CLASSES 64
/* one scene's centres, confidences, distances and assignments live in the rows kernel's LDS: 68 bytes per proposal */
#define OMNIPQ_MT_MAX_K 512
/* the b * k values of one clipped array are selected from in the clip kernel's LDS, 4 bytes each: 60 KiB */
#define OMNIPQ_MT_MAX_ROWS 15360
#define OMNIPQ_MT_TERMS 10

typedef struct {
  int prefixes, b, k, nc, ns;
  /* the student's outputs, one pointer per prefix */
  const float *center[OMNIPQ_MT_MAX_PREFIXES];              /* (b, k, 3) */
  const float *objectness_scores[OMNIPQ_MT_MAX_PREFIXES];   /* (b, k, 2) */
  const float *sem_cls_scores[OMNIPQ_MT_MAX_PREFIXES];      /* (b, k, nc) */
  const float *size_scores[OMNIPQ_MT_MAX_PREFIXES];         /* (b, k, ns) */
  const float *size_residuals[OMNIPQ_MT_MAX_PREFIXES];      /* (b, k, ns, 3) */
  const float *quad_center[OMNIPQ_MT_MAX_PREFIXES];         /* (b, k, 3) */
  const float *quad_scores[OMNIPQ_MT_MAX_PREFIXES];         /* (b, k, 2) */
  const float *normal_vector[OMNIPQ_MT_MAX_PREFIXES];       /* (b, k, 3) */
  const float *quad_size[OMNIPQ_MT_MAX_PREFIXES];           /* (b, k, 2) */
  /* the teacher's (its objectness_scores are not read) */
  const float *t_center[OMNIPQ_MT_MAX_PREFIXES];
  const float *t_sem_cls_scores[OMNIPQ_MT_MAX_PREFIXES];
  const float *t_size_scores[OMNIPQ_MT_MAX_PREFIXES];
  const float *t_size_residuals[OMNIPQ_MT_MAX_PREFIXES];
  const float *t_quad_center[OMNIPQ_MT_MAX_PREFIXES];
  const float *t_quad_scores[OMNIPQ_MT_MAX_PREFIXES];
  const float *t_normal_vector[OMNIPQ_MT_MAX_PREFIXES];
  const float *t_quad_size[OMNIPQ_MT_MAX_PREFIXES];
  /* the augmentation of the student's input relative to the teacher's (train.py:526-529) and the size templates */
  const int *flip_x;                                        /* (b) */
  const int *flip_y;                                        /* (b) */
  const float *rot_mat;                                     /* (b, 3, 3) */
  const float *scale;                                       /* (b) */
  const float *mean_size;                                   /* (ns, 3) */
} omnipq_mt_desc;

typedef struct {
  float *center[OMNIPQ_MT_MAX_PREFIXES];
  float *objectness_scores[OMNIPQ_MT_MAX_PREFIXES];
  float *sem_cls_scores[OMNIPQ_MT_MAX_PREFIXES];
  float *size_residuals[OMNIPQ_MT_MAX_PREFIXES];
  float *quad_center[OMNIPQ_MT_MAX_PREFIXES];
  float *quad_scores[OMNIPQ_MT_MAX_PREFIXES];
  float *normal_vector[OMNIPQ_MT_MAX_PREFIXES];
  float *quad_size[OMNIPQ_MT_MAX_PREFIXES];
} omnipq_mt_grads;

/* bytes of the workspace the forward fills and the backward reads (values, assignments, classes, masks, records); 0 for
 * arguments the forward would refuse */
long long omnipq_mt_consistency_workspace_bytes(int prefixes, int b, int k);

/* ema_center float[prefixes][2][b][k][3], assignment long long[prefixes][2][b][k] (ind2), confidence float[prefixes][2][b][k],
 * terms float[OMNIPQ_MT_TERMS]: all overwritten.  The inputs are left untouched. */
int omnipq_mt_consistency(const omnipq_mt_desc *d, float *ema_center, long long *assignment, float *confidence,
                          void *workspace, float *terms, void *stream);

/* g_terms float[OMNIPQ_MT_TERMS] = dLoss/dterms, folded with the term weights above -> the gradients of the student's
 * center, objectness_scores, sem_cls_scores, size_residuals, quad_center, quad_scores, normal_vector and quad_size of every
 * prefix, each overwritten in full (size_residuals: zero outside the arg-max class; normal_vector: zero in z).  Nothing flows
 * to the teacher, to size_scores or through any eps.  The masks are the forward's (read from the workspace), not recomputed. */
int omnipq_mt_consistency_grad(const omnipq_mt_desc *d, const void *workspace, const float *g_terms,
                               const omnipq_mt_grads *g, void *stream);

/* ---- ARKit physical-constraint loss ------------------------------------------------------------------------------------
 * Reference: models/utils/arkit_loss_util.py:5-52 `get_arkit_pc_loss(end_points, batch_data_unlabeled, DATASET_CONFIG)` with
 * models/loss_helper_pq.py:307-350 (`get_2d_box`, `projection2d`), called by train.py:537: the ground-truth boxes of the
 * UNLABELLED scenes must not poke through the quads predicted for them.  There it is a Python loop over B x 256 quads with a
 * host read (`if quad_scores[b, k] > 0.1`) and about twenty small ops each.
 *
 * The full batch holds first + b scenes; the predictions read are those of scenes [first, first + b) (the reference's
 * `[batch_size:]`, first = b = the number of unlabelled scenes), the labels are the unlabelled batch's own:
 *   quad_center, normal_vector (first + b, q, 3); quad_size, quad_scores (first + b, q, 2)           f32
 *   center_label, size_label (b, k2, 3) f32; num_gt_boxes: the count n_s of scene s is num_gt_boxes[s * count_stride]
 *   (int64; a strided view such as `num_gt_boxes[..., 0]` needs no copy)
 * Per unlabelled scene s and quad j, c = quad_center[j], n = normal_vector[j]:
 *   gate_j  = softmax(quad_scores[j])[1] > 0.1                                                        (no gradient)
 *   rev_j   = -(c.x n.x + c.y n.y) < 0          (the normal points away from the pseudo scene centre; c detached: no gradient)
 *   (a, b)  = rev_j ? -(n.x, n.y) : (n.x, n.y)                                     NOT normalised, as in the reference
 *   corners : for every box i < min(n_s, k2) the four points p = (g.x +- l / 2, g.y +- w / 2), g = center_label[i],
 *             (l, w) = size_label[i][:2], in the order (+, +), (+, -), (-, +), (-, -)
 *   delta   = a p.x + b p.y - (a c.x + b c.y)
 *   t       = p - (a, b) delta;  inside = |t - c.xy| < quad_size[j][0]                                 (no gradient)
 *   pair    = relu(-delta) * inside                                                                    relu'(0) = 0
 *   loss   += gate_j * sum_p pair / n_s;   collisions += gate_j * #{p : pair > 1e-4}
 * loss is the sum over scenes and quads; there is no division by the batch size, as in the reference.
 *
 * Differences from the reference, on purpose:
 *   - a scene with n_s <= 0 contributes 0 to both outputs (the reference: 0 / 0, NaN as soon as one quad passes the gate);
 *   - rows i >= n_s of the labels are never read (they may hold NaN);
 *   - arithmetic per pair is f64 from the f32 inputs (the reference: f32); per-quad sums in corner order, a fixed-order sum
 *     over the workgroup, then over the scenes in scene order: the same inputs give the same bits;
 *   - the inputs are left untouched.
 * No float atomics, no host read.  Forward: two launches (one workgroup per scene with the scene's boxes in LDS, 16 bytes
 * per box, one thread per quad looping over the corners and over the quads beyond 256; a one-wave fold).  Backward: one launch,
 * grid (first + b), which re-evaluates the forward's per-pair functions (compiled without FP contraction: the same decisions)
 * on the quads whose record shows live pairs.
 *
 * record: int[b][q][OMNIPQ_ARKIT_RECORD_INTS] = {gate, rev, pairs inside, pairs inside with delta < 0, collisions}; a quad
 * that does not pass the gate has {0, 0, 0, 0, 0}.  scene_sums: double[b][2], the scenes' (loss, collisions) between the
 * two launches.  out: float[2] = (loss, collisions).  All three are overwritten.
 *
 * OMNIPQ_EINVAL: a null required pointer, b < 0, first < 0, q < 1, k2 < 1, count_stride < 1.  OMNIPQ_ETOOLARGE:
 * k2 > OMNIPQ_ARKIT_MAX_BOXES, or (first + b) * q * OMNIPQ_ARKIT_RECORD_INTS beyond 2^31.  b == 0 succeeds and does nothing. */
#define OMNIPQ_ARKIT_MAX_BOXES 256
#define OMNIPQ_ARKIT_RECORD_INTS 5

int omnipq_arkit_pc(int first, int b, int q, int k2, const float *quad_center, const float *normal_vector,
                    const float *quad_size, const float *quad_scores, const float *center_label, const float *size_label,
                    const long long *num_gt_boxes, long long count_stride, int *record, double *scene_sums, float *out,
                    void *stream);

/* g_out float[1] = dLoss/dloss -> g_quad_center, g_normal_vector (first + b, q, 3): every element is written exactly once by
 * this launch -- zero for the scenes below `first` and in z; in x and y of the unlabelled scenes, with S = the pairs inside
 * with delta < 0 and sgn = rev_j ? -1 : 1,
 *   d loss / d c.xy = gate_j |S| (a, b) / n_s;      d loss / d n.xy = -gate_j sgn sum_S (p - c.xy) / n_s.
 * Nothing flows to quad_scores, quad_size or the labels. */
int omnipq_arkit_pc_grad(int first, int b, int q, int k2, const float *quad_center, const float *normal_vector,
                         const float *quad_size, const float *quad_scores, const float *center_label, const float *size_label,
                         const long long *num_gt_boxes, long long count_stride, const int *record, const float *g_out,
                         float *g_quad_center, float *g_normal_vector, void *stream);

#ifdef __cplusplus
}
#endif
#endif
