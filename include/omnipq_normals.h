/* omnipq_normals.h -- C ABI of the per-point normal estimation: k nearest neighbours, plane fit, smoothing, orientation.
 *
 * Replaces the offline step of the reference's data preparation (scannet/compute_normal_for_pc.py:29-48,
 * ARKitScenes/dataset/compute_normal_for_pc.py:25-38): the cloud is written to a text file, MeshLab's
 * `compute_normals_for_point_sets` runs with k = 100, smoothiter = 5, flipflag = True, viewpos = pc_center, and every normal is
 * then flipped so that (p - pc_center) . n >= 0.  MeshLab is not part of this project: the four stages below are THIS
 * library's contract (plane fit over the k nearest, sign-aligned neighbour averaging, viewpoint flip); agreement with MeshLab's
 * output has not been checked.  The final orientation does not depend on the filter: after the reference's own flip
 * (:44-47) it is (p - c) . n >= 0 whatever the filter did.
 *
 * Conventions as in omnipq_pointops.h: device pointers, dense row-major tensors, a hipStream_t, int return (0 = ok), nothing
 * synchronises and nothing is read back.  Limits: 1 <= k <= 128, b <= 65535.  Coordinates must be finite.
 * Every entry point returns OMNIPQ_EINVAL for a negative size, k outside [1, 128], b > 65535, a cell that is not > 0 (NaN
 * included) or a NULL pointer it needs, before anything is launched; a zero b, n (m for omnipq_knn) is OMNIPQ_OK and launches
 * nothing.  The kernels do not depend on the library's 16-bit element type.
 *
 * 1. Neighbours.  N(i) = the k points of xyz with the smallest (d2, index), lexicographic; d2 in f32 exactly as the numerics
 *    contract of omnipq_pointops.h states it, fma(dz, dz, fma(dx, dx, fl(dy * dy))) on d = query - point.  The point itself is
 *    included (d2 = 0).  Rows are stored ascending in that order; with n < k the tail of a row is -1 / +inf.
 * 2. Plane fit.  Over the row's valid points, in row order, f64, nothing contracted: mean = (sum p) / cnt, then
 *    C = (sum (p - mean)(p - mean)^T) / cnt.  Cyclic Jacobi, 10 sweeps over (0,1), (0,2), (1,2); the column of the smallest
 *    eigenvalue (the first among equal ones), rounded to f32, then negated if its component of largest magnitude (the first
 *    among equal ones) is negative.  A degenerate neighbourhood yields a finite unit vector, which one is unspecified.
 * 3. Smoothing step.  t_i = sum over j in row i, in order, of s_ij n_j with s_ij = +1 if ((n_i.x n_j.x + n_i.y n_j.y) +
 *    n_i.z n_j.z) > 0 else -1, everything f64 on the f32 inputs; out_i = f32(t_i / sqrt((t.x t.x + t.y t.y) + t.z t.z)), or
 *    n_i where t_i = 0; entries < 0 are skipped.
 * 4. Orientation.  n_i <- -n_i iff ((p.x - c.x) n.x + (p.y - c.y) n.y) + (p.z - c.z) n.z < 0 in f64.
 */
#ifndef OMNIPQ_NORMALS_H
#define OMNIPQ_NORMALS_H
#ifdef __cplusplus
extern "C" {
#endif

/* Stage 1 for m queries new_xyz (b, m, 3) f32 against xyz (b, n, 3) f32: idx (b, m, k) int32, dist2 (b, m, k) f32 or NULL.
 * `cell` is the edge of the hash grid's cells: it changes the time, never the result (a query the grid cannot answer --
 * fewer than k points within three shells of cells, coordinates beyond 2000 cells -- walks all n points instead).  workspace: omnipq_knn_workspace_bytes(b, n, m) bytes of device memory (< 0: negative size). */
long long omnipq_knn_workspace_bytes(int b, int n, int m);
int omnipq_knn(int b, int n, int m, int k, float cell, const float *new_xyz, const float *xyz, int *idx, float *dist2,
               void *workspace, void *stream);

/* Stage 2: idx (b, n, k) as omnipq_knn leaves it (entries < 0 or >= n are skipped) -> normals_out (b, n, 3) f32 and, unless
 * NULL, eig_out (b, n, 3) f64, the eigenvalues of C ascending. */
int omnipq_normals_plane_fit(int b, int n, int k, const float *xyz, const int *idx, float *normals_out, double *eig_out,
                             void *stream);

/* Stage 3, one step: normals_in (b, n, 3) f32 -> normals_out (b, n, 3) f32, which must not overlap. */
int omnipq_normals_smooth(int b, int n, int k, const int *idx, const float *normals_in, float *normals_out, void *stream);

/* Stage 4 in place: centre (b, 3) f64 in device memory (compute_normal_for_pc.py:34-35 and :44-47). */
int omnipq_normals_orient(int b, int n, const float *xyz, const double *centre, float *normals, void *stream);

/* The four stages chained (k neighbours of every point among the scene's own points, `iters` >= 0 smoothing steps): the bits
 * of the stage calls above.  workspace: omnipq_estimate_normals_workspace_bytes(b, n, k) bytes (< 0: a size out of range). */
long long omnipq_estimate_normals_workspace_bytes(int b, int n, int k);
int omnipq_estimate_normals(int b, int n, int k, int iters, float cell, const float *xyz, const double *centre,
                            float *normals_out, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
