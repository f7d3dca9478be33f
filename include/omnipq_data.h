/* omnipq_data.h -- C ABI of the device-resident input side: a batch of training items sampled, augmented and labelled
 * from scenes that live in device memory.
 *
 * Reference: scannet/scannet_detection_dataset.py:86-312 and ARKitScenes/arkitscenes_dataset.py:83-233, the datasets'
 * `__getitem__`: two sub-samplings of the scene (student, teacher), flip / rotate / scale of points, normals, boxes and
 * quads, and the vote labels from the extent of every instance among the sampled points.  There it is host work per item;
 * here the scenes are uploaded once into one packed arena and a whole batch is four launches (two for the unlabelled
 * flavour), no host read, every launch capturable:
 *   labels   grid (b): the scene's box / quad labels and per-item scalars, the float64 box centres for the vote assignment,
 *            and the reset of the scene's extent table
 *   points   grid (ceil(k / 1024), b): per tile of positions the teacher's rows (draw, gather), then the student's (draw,
 *            gather, augment, instance extents: integer min / max on an order-preserving encoding, folded in LDS, then one
 *            global atomic per (workgroup, instance, word)); the unlabelled flavour's instantiation carries no LDS
 *   instance grid (b): per instance the centre, the `ind[0]` validity rule and the nearest box centre
 *   votes    grid (ceil(k / 256), b): per point vote, mask and instance label
 *
 * Conventions as in omnipq_semi.h: device pointers, sizes, a hipStream_t, int return (0 = ok); arguments are validated before
 * the device is touched; b == 0 succeeds and does nothing.  The three structs are HOST memory holding device pointers.
 *
 * Draw.  Position p of scene slot s of the batch, stream t (0 student, 1 teacher), scene of n rows:
 *   key  = mix64(*seed ^ mix64(((t << 32) | s) + 1)),  mix64 = the splitmix64 finaliser of (x + 0x9E3779B97F4A7C15)
 *   rk_r = low 32 bits of mix64(key + r), r = 0..OMNIPQ_ASM_ROUNDS-1
 *   n >= k  a permutation of [0, n) evaluated at p: balanced Feistel network over 2h bits (h = the smallest integer >= 1
 *           with 4^h >= n), (L, R) <- (R, L ^ (fmix32(R ^ rk_r) & (2^h - 1))) per round, x = (L << h) | R, walked along its cycle
 *           until x < n: distinct positions give distinct rows, no table, one thread per position
 *   n <  k  with replacement: (fmix32(p ^ rk_0) ^ rk_1, fmix32 again) * n >> 32
 *   fmix32 = murmur3's finaliser.  `seed` is a 64-bit word in device memory read by the kernel: the same word gives the same
 *   draws, a replay that finds it advanced draws afresh.  The caller may supply either index array instead; a supplied index
 *   outside [0, n) is never used to read: its row is written as zeros with vote mask 0 and instance label -1.
 *
 * Points (student).  Row (x, y, z, ...) f32: x negated when flip_x, y when flip_y; rotation in f64 from the host's f64 matrix
 * R as x R00 + y R01 and x R10 + y R11 (plain multiplies and adds, no contraction), rounded to f32; then an f32 multiply by
 * (float)scale of x, y, z and of the height column.  Other columns are copied.  Identity parameters (no flip, R = I exactly,
 * scale = 1: the evaluation loader) copy the rows as stored, as the reference leaves them, so a -0.0 stays -0.0.  Normals: flipped and rotated the same way,
 * not scaled (flavour 1: copied as stored).  Teacher rows are copied as stored.
 *
 * Instances (flavour 0).  Per dense instance id g < I of the scene: min and max of the augmented x, y, z and the smallest
 * sampled position `first` over the sampled points of g; centre = 0.5f * (min + max) in f32; valid iff the semantic label
 * of the point at `first` is in nyu40ids; ilabel = argmin_j sum_d ((double)centre_d - C_jd)^2 over the 64 f64 box centres
 * C (padding rows at +1000 after augmentation), the lowest index on ties.  vote = centre - x in f32, three times.
 *
 * Boxes and quads: f64 throughout, rounded once to f32.  Box (c, l): c flipped, c' = R c, l'_x = 2 max over the four corners
 * (+-l_x / 2, +-l_y / 2) of their rotated x, l'_y likewise, l'_z = l_z, both times scale (model_util_scannet.py:73-95).
 * Quad: centre and normal flipped and rotated, centre and size scaled (:97-103).  Horizontal quads: flipped, rotated, scaled.
 *
 * OMNIPQ_EINVAL: a null struct or required pointer, b < 0, k < 1, scenes < 1, rows_total < 0, pitch < 3, height_col neither -1 nor in
 * [3, pitch), flavour outside {0, 1}, n_ids < 0, n_sizes < 1 (flavour 0), no seed although an index array is missing.
 * OMNIPQ_ETOOLARGE: b > OMNIPQ_ASM_MAX_BATCH, k > OMNIPQ_ASM_MAX_K, pitch > OMNIPQ_ASM_MAX_PITCH, n_ids > OMNIPQ_ASM_MAX_IDS.
 */
#ifndef OMNIPQ_DATA_H
#define OMNIPQ_DATA_H
#ifdef __cplusplus
extern "C" {
#endif

#define OMNIPQ_ASM_MAX_OBJ 64
#define OMNIPQ_ASM_MAX_QUAD 32
#define OMNIPQ_ASM_MAX_HQUAD 4
#define OMNIPQ_ASM_NUM_PROPOSAL 256
#define OMNIPQ_ASM_MAX_INSTANCES 1024
#define OMNIPQ_ASM_MAX_BATCH 65535
#define OMNIPQ_ASM_MAX_K 16777216
#define OMNIPQ_ASM_MAX_PITCH 8
#define OMNIPQ_ASM_MAX_IDS 64
#define OMNIPQ_ASM_ROUNDS 6
/* ints per scene of `meta`: rows, instances, boxes, rectangles, total_quad_num, horizontal quads, 2 spare */
#define OMNIPQ_ASM_META_INTS 8
/* doubles per scene of `labels`: boxes [64][7] (centre, size, class index), rectangles [32][8] (centre, normal, size),
 * horizontal quads [4][4][3] */
#define OMNIPQ_ASM_LABEL_DOUBLES 752
/* doubles per item of `params`: flip_x, flip_y (0 / 1), rot_mat [3][3], scale */
#define OMNIPQ_ASM_PARAM_DOUBLES 12

typedef struct {
  int scenes, pitch, height_col;   /* height_col: the column scaled with the coordinates, or -1 */
  long long rows_total;            /* rows of the arena: a scene whose table entry leaves [0, rows_total) counts as empty */
  const float *points;             /* (rows_total, pitch) */
  const float *normals;            /* (rows_total, 3) */
  const float *colors;             /* (rows_total, 3), or NULL */
  const int *instance;             /* (rows_total) dense ids in [0, I); flavour 0 */
  const int *semantic;             /* (rows_total); flavour 0 */
  const long long *row_offset;     /* (scenes) */
  const int *meta;                 /* (scenes, OMNIPQ_ASM_META_INTS) */
  const double *labels;            /* (scenes, OMNIPQ_ASM_LABEL_DOUBLES) */
} omnipq_asm_bank;

typedef struct {
  int b, k, flavour;               /* flavour: 0 labelled (ScanNet item), 1 unlabelled (ARKit item) */
  int n_ids, n_sizes;
  const int *scene_slot;           /* (b); a slot outside [0, scenes) counts as an empty scene */
  const double *params;            /* (b, OMNIPQ_ASM_PARAM_DOUBLES) */
  const unsigned long long *seed;  /* one word; may be NULL when both index arrays are supplied */
  const int *choices_in;           /* (b, k) or NULL: draw */
  const int *ema_choices_in;       /* (b, k) or NULL: draw */
  const int *nyu40ids;             /* (n_ids); flavour 0 */
  const double *mean_size;         /* (n_sizes, 3); flavour 0 */
} omnipq_asm_batch;

/* Every array is overwritten in full.  [0]: flavour 0 only (may be NULL otherwise); [1]: flavour 1 only. */
typedef struct {
  float *point_clouds;             /* (b, k, pitch) */
  float *vertex_normals;           /* (b, k, 3) */
  float *ema_point_clouds;         /* (b, k, pitch) */
  int *choices;                    /* (b, k) */
  int *ema_choices;                /* (b, k) */
  float *semantic_labels;          /* (b, k) [0] */
  float *pcl_color;                /* (b, k, 3) [0], or NULL */
  float *vote_label;               /* (b, k, 9) [0] */
  long long *vote_label_mask;      /* (b, k) [0] */
  long long *point_instance_label; /* (b, k) [0] */
  float *center_label;             /* (b, 64, 3) */
  long long *heading_class_label;  /* (b, 64) zeros */
  float *heading_residual_label;   /* (b, 64) zeros */
  long long *size_class_label;     /* (b, 64) [0] */
  float *size_residual_label;      /* (b, 64, 3) [0] */
  float *size_gts;                 /* (b, 64, 3) [0] */
  float *size_label;               /* (b, 64, 3) [1] */
  long long *sem_cls_label;        /* (b, 64) [0] */
  float *box_label_mask;           /* (b, 64) [0] */
  long long *num_gt_boxes;         /* (b, 256) */
  float *gt_quad_centers;          /* (b, 32, 3) [0] */
  float *gt_normal_vectors;        /* (b, 32, 3) [0] */
  float *gt_quad_sizes;            /* (b, 32, 2) [0] */
  long long *num_gt_quads;         /* (b, 256) [0] */
  long long *num_total_quads;      /* (b, 256) [0] */
  float *horizontal_quads;         /* (b, 4, 4, 3) [0] */
  long long *flip_x_axis;          /* (b); flavour 1 reports arkitscenes_dataset.py:153-165: flip_x && !flip_y */
  long long *flip_y_axis;          /* (b); flavour 1: 0 */
  float *rot_mat;                  /* (b, 3, 3) */
  float *scale;                    /* (b) */
  long long *scan_idx;             /* (b) [0]: the scene slot */
} omnipq_asm_out;

/* bytes of the workspace a batch of b items needs (extent table, instance table, f64 box centres); 0 for b outside
 * [1, OMNIPQ_ASM_MAX_BATCH] */
long long omnipq_assemble_workspace_bytes(int b);

int omnipq_assemble_batch(const omnipq_asm_bank *bank, const omnipq_asm_batch *batch, const omnipq_asm_out *out,
                          void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
