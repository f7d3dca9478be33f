/* omnipq_eval.h -- C ABI of the evaluation-side consumer of the layout branch.
 *
 * Reference: models/ap_helper_pq.py:323-460 `parse_quad_predictions` and :462-517 `parse_quad_groundtruths`, which turn
 * (quad_center, normal_vector, quad_size, quad_scores) into thin oriented boxes, suppress overlapping ones
 * (utils/nms.py:77-113 `nms_3d_faster` on the boxes' axis-aligned extents) and hand Python lists to QUADAPCalculator.
 * There every proposal is a Python iteration with ~10 `.detach().cpu().numpy()` reads (B x 256 of them per head and
 * batch); here one launch decodes all proposals of the batch and one launch runs the greedy suppression of every scene,
 * and the host reads the results back once.  The packed detections (omnipq_decode_boxes .. omnipq_pack_quads) leave the same
 * results on the device, and omnipq_layout_f1 scores the packed quads there: QUADAPCalculator.compute_F1 (:695-736), the number
 * an evaluation epoch returns, as five integers read once per epoch.
 * Conventions as in omnipq_pointops.h: device pointers, sizes, a hipStream_t, int return (0 = ok).
 */
#ifndef OMNIPQ_EVAL_H
#define OMNIPQ_EVAL_H
#ifdef __cplusplus
extern "C" {
#endif

/* Per proposal (b, k) of quad_center (b, k, 3), normal_vector (b, k, 3), quad_size (b, k, 2) [width, height], all f32:
 *   heading = acos(n_y / |n|), mirrored to 2 pi - heading when n_x > 0         (f32, as the reference's torch ops; :364-368)
 *   corners8 (b, k, 8, 3) f64: get_3d_box((width, length, height), heading, centre in the upright-camera frame
 *                              (x, -z, y))                                      (utils/box_util.py:218-233; f64 as numpy)
 *   aabb     (b, k, 6)    f64: min / max of the eight corners per axis         (:409-414: the NMS input)
 *   verts4   (b, k, 4, 3) f32: get_verts(centre, width, height, normal)        (:270-296: the corners the F1 score compares)
 *   prob     (b, k)       f32: softmax(quad_scores)[..., 1]; quad_scores (b, k, 2) may be NULL (ground truth: prob untouched)
 * Any output may be NULL. */
int omnipq_parse_quads(int b, int k, const float *quad_center, const float *normal_vector, const float *quad_size,
                       const float *quad_scores, float length, double *corners8, double *aabb, float *verts4, float *prob,
                       void *stream);

/* Greedy 3D non-maximum suppression of utils/nms.py:77-113, one scene per workgroup: visit the boxes by decreasing score
 * (the higher index first among equal scores), keep a box unless an already kept one overlaps it by more than
 * `overlap_threshold` -- IoU of the axis-aligned extents, or intersection / own volume with `old_type` != 0.
 * aabb (b, k, 6) f64 (x1, y1, z1, x2, y2, z2), score (b, k) f32, valid (b, k) u8 or NULL (only valid boxes take part),
 * keep (b, k) u8: 1 = picked.  k <= 4096. */
int omnipq_nms3d(int b, int k, const double *aabb, const float *score, const unsigned char *valid,
                 double overlap_threshold, int old_type, unsigned char *keep, void *stream);

/* The same with suppression restricted to boxes of the same class (utils/nms.py:115-158 `nms_3d_faster_samecls`):
 * cls (b, k) int32.  2D suppression (`nms_2d_faster`, :44-75) is this kernel on extents whose second axis is [0, 1]. */
int omnipq_nms3d_samecls(int b, int k, const double *aabb, const float *score, const unsigned char *valid, const int *cls,
                         double overlap_threshold, int old_type, unsigned char *keep, void *stream);

/* Corners (n, 8, 3) f64 in the upright-camera frame and extents (n, 6) f64 of n oriented boxes, utils/box_util.py:218-233
 * `get_3d_box(box_size, heading_angle, center)`: center (n, 3) f32 in the depth frame (flipped here as
 * ap_helper_pq.py:24-32 does), size (n, 3) f64 (l, w, h), heading (n) f32 or NULL (axis aligned).  For the object half of
 * the evaluation (models/ap_helper_pq.py:73-266 `parse_predictions`, `parse_groundtruths`). */
int omnipq_box_corners(long long n, const float *center, const double *size, const float *heading, double *corners8,
                       double *aabb, void *stream);

/* nonempty (b, k) u8 = the box holds at least min_points of its scene's points xyz (b, n, 3) -- `remove_empty_box`,
 * ap_helper_pq.py:127-139, where every box costs a Delaunay triangulation and a point-location query over the scene. */
int omnipq_points_in_boxes(int b, int n, int k, const float *xyz, const float *center, const double *size,
                           const float *heading, int min_points, unsigned char *nonempty, void *stream);

/* Oriented-box IoU of the detection metrics (utils/box_util.py:93-118 `box3d_iou`, as omni-pq_amd/eval_det.py restates it;
 * csrc/eval_iou.hip).  A box is its corners (8, 3) f64 in get_3d_box's layout: rows 0-3 the top face, 4-7 the bottom face,
 * up = -Y.  Everything is f64 and nothing is contracted: the footprints (x, z) of corners 3, 2, 1, 0 are clipped with the
 * host's strict `inside` test and the host's intersection point (n1, n2, the reciprocal n3, two multiplications), the areas
 * are shoelace areas, the heights and volumes are formed as on the host.  Only the order in which the shoelace sums add
 * their terms differs from numpy's dot.
 *
 * Elementwise: iou3d[i], iou2d[i] (n) of a8[i] against b8[i] ((n, 8, 3) each; a8 is box3d_iou's first argument).  Either
 * output may be NULL, not both. */
int omnipq_obb_iou_pairs(long long n, const double *a8, const double *b8, double *iou3d, double *iou2d, void *stream);

/* The inner loop of utils/eval_det.py:75-161 `eval_det_cls` for every detection at once.  Detection i, pred8 (n_pred, 8, 3),
 * belongs to segment pred_seg[i] in [0, n_seg) -- one (class, scan) group -- whose ground-truth boxes are
 * gt8[seg_start[s] .. seg_start[s + 1]) of gt8 (n_gt, 8, 3); seg_start has n_seg + 1 entries.  Per detection: start at
 * (-inf, -1), visit the segment's boxes in order, replace on iou3d(pred, gt) > ovmax.  So the first maximum wins among equal
 * values, a NaN overlap never wins, an empty segment yields (-inf, -1).  ovmax (n_pred) f64, jmax (n_pred) int32: the index
 * WITHIN the segment.  The greedy matching that consumes the two stays on the host (eval_det.match_from_best). */
int omnipq_obb_iou_best(long long n_pred, const double *pred8, const int *pred_seg, int n_seg, const long long *seg_start,
                        long long n_gt, const double *gt8, double *ovmax, int *jmax, void *stream);

/* ---- packed detections (csrc/detect.hip) ---------------------------------------------------------------
 * What models/ap_helper_pq.py:73-236 `parse_predictions` computes in front of the suppression, for all b * k proposals in one
 * launch, one thread per proposal.  Inputs f32, contiguous: center (b, k, 3), heading_scores / heading_residuals (b, k, nh),
 * size_scores (b, k, ns), size_residuals (b, k, ns, 3), sem_cls_scores (b, k, ncls), objectness_scores (b, k, 2); mean_size
 * (ns, 3) f64.  heading_rule: 0 = the dataset's class2angle returns 0 (axis-aligned boxes), 1 = class * 2 pi / nh + residual
 * folded into (-pi, pi].  Outputs:
 *   heading_cls, size_cls, sem_cls (b, k) i32   the first maximum of the row; a NaN counts as larger than every number, the
 *                                               first NaN wins (torch.argmax on the device)
 *   size     (b, k, 3) f64   mean_size[size_cls] + (double)residual[size_cls]
 *   heading  (b, k)    f32   rule 1: (float)(a > pi ? a - 2 pi : a), a = (double)cls * (2 pi / nh) + (double)residual[cls],
 *                            product and sum rounded separately; rule 0: 0
 *   obj_prob (b, k)    f32   1 / (1 + exp(-logit 1)) evaluated in f64, rounded once
 *   sem_prob (b, k, ncls) f32 or NULL   softmax in f64 (row maximum subtracted, sum in index order), rounded once
 *   corners8 (b, k, 8, 3) f64, aabb (b, k, 6) f64   as omnipq_box_corners (the same device function); with bev != 0 the
 *                            second axis of aabb is [0, 1]: bird's-eye-view suppression through omnipq_nms3d*
 * Every output but sem_prob is required.  nh, ns, ncls in [1, omnipq_decode_boxes_max_classes()], k <= 4096 (the limit of
 * omnipq_nms3d); anything else is OMNIPQ_EINVAL.  b == 0 or k == 0: nothing is launched. */
int omnipq_decode_boxes(int b, int k, int nh, int ns, int ncls, const float *center, const float *heading_scores,
                        const float *heading_residuals, const float *size_scores, const float *size_residuals,
                        const float *sem_cls_scores, const float *objectness_scores, const double *mean_size,
                        int heading_rule, int bev, int *heading_cls, int *size_cls, int *sem_cls, double *size,
                        float *heading, float *obj_prob, float *sem_prob, double *corners8, double *aabb, void *stream);

/* The largest nh, ns and ncls omnipq_decode_boxes and omnipq_pack_boxes accept (host only). */
int omnipq_decode_boxes_max_classes(void);

/* Stable compaction of the proposals a scene keeps, one workgroup per scene, no atomics.  Proposal j of scene s is selected
 * when keep[s, j] != 0 && score[s, j] > conf (strict, f32); the selected ones are written in increasing j to rows
 * [0, count[s]) of the outputs:
 *   count (b) i32; index (b, k) i32 = j; out_cls (b, k) i32 = cls[s, j]; out_score (b, k) f32 = score[s, j];
 *   out_corners8 (b, k, 8, 3) f64 = corners8[s, j]; out_sem_prob (b, k, ncls) f32 = sem_prob[s, j] (both NULL: not wanted)
 * Rows [count[s], k) hold index -1 and zeros everywhere else, so every output byte is a function of the inputs.
 * keep (b, k) u8, score (b, k) f32, cls (b, k) i32, corners8 (b, k, 8, 3) f64.  k <= 4096, ncls as above (ignored without
 * sem_prob); anything else, or sem_prob without out_sem_prob, is OMNIPQ_EINVAL.  b == 0 or k == 0: nothing is launched. */
int omnipq_pack_boxes(int b, int k, int ncls, const unsigned char *keep, const float *score, float conf, const int *cls,
                      const double *corners8, const float *sem_prob, int *count, int *index, int *out_cls, float *out_score,
                      double *out_corners8, float *out_sem_prob, void *stream);

/* The same for the quads, on the outputs of omnipq_parse_quads and omnipq_nms3d, two lists per scene:
 *   the AP list  keep && prob > conf:        count (b), index (b, k), out_score (b, k) f32, out_corners8 (b, k, 8, 3) f64
 *   the F1 list  keep && prob > quad_thres:  count_f1 (b), index_f1 (b, k), out_verts4 (b, k, 4, 3) f32
 * Tail rows as above.  k <= 4096. */
int omnipq_pack_quads(int b, int k, const unsigned char *keep, const float *prob, float conf, float quad_thres,
                      const double *corners8, const float *verts4, int *count, int *index, float *out_score,
                      double *out_corners8, int *count_f1, int *index_f1, float *out_verts4, void *stream);

/* ---- layout F1 (csrc/layout_f1.hip) ------------------------------------------------------------------------
 * The counts of models/ap_helper_pq.py:695-736 `QUADAPCalculator.compute_F1` for a batch, one workgroup per scene, on the F1
 * list omnipq_pack_quads wrote.  The rule is the reference's as it stands:
 *   ground-truth list of scene s   rows j in [0, g) of gt_verts4[s] with j < num_total[s, min(j, num_total_cols - 1)], in
 *                                  increasing j (parse_quad_groundtruths with num_total_quads); npos = its length
 *   two corners are the same       sqrt((dx dx + dy dy) + dz dz) <= same_thres, both corners widened from f32 to f64, every
 *                                  product and sum rounded on its own; a NaN never passes
 *   a predicted quad is correct    when some quad G of the list has all four dist(P[i], G[i]) or all four dist(P[i], G[i ^ 1])
 *                                  (the order [1, 0, 3, 2]) within same_thres: tp_wall += 1, otherwise fp += 1; an empty list
 *                                  makes every quad a false positive
 *   ceiling and floor              get_ceiling_and_floor (:673-693) appends one entry per visited corner in BOTH branches, so
 *                                  its `len(...) == 4` test holds exactly when the scene has two predicted quads.  Only then:
 *                                  the ceiling list is corners 0, 1 of quad 0 and then of quad 1, the floor list corners 2, 3;
 *                                  a corner is appended as it is when no earlier entry of its list is within same_thres, and
 *                                  otherwise as the f32 midpoint (p + corner) / 2 with the FIRST such entry p; each list is
 *                                  scored as a quad against ALL h rows of horizontal[s] -- the zero padding rows included, as
 *                                  on the host -- and adds 1 to tp_horizontal when correct, never to fp
 * verts4 (b, k, 4, 3) f32: rows [0, count_f1[s]) are read, count_f1 (b) i32 clamped to [0, k]; gt_verts4 (b, g, 4, 3) f32;
 * num_total (b, num_total_cols) i64; horizontal (b, h, 4, 3) f32, h may be 0.
 *   per_scene (b, 4) i32   written: [tp_wall, fp, npos, tp_horizontal]
 *   acc       (5)    i64   incremented by the batch's four sums and by b scans: integer atomics, so the result does not
 *                          depend on their order
 * Either output may be NULL, not both.  k <= 4096, g <= omnipq_layout_f1_max_gt(), h <= 8, num_total_cols >= 1, same_thres
 * finite and >= 0; anything else, or a missing pointer of a non-empty array, is OMNIPQ_EINVAL before the device is touched.
 * b == 0 launches nothing.  The F1 itself stays a host expression over the five integers (ap_helper_pq.LayoutF1). */
int omnipq_layout_f1(int b, int k, const int *count_f1, const float *verts4, int g, const float *gt_verts4,
                     const long long *num_total, int num_total_cols, int h, const float *horizontal, double same_thres,
                     int *per_scene, long long *acc, void *stream);

/* The largest g omnipq_layout_f1 accepts (host only). */
int omnipq_layout_f1_max_gt(void);

#ifdef __cplusplus
}
#endif
#endif
