"""Per-point normals on the device (csrc/point_normals.hip, include/omnipq_normals.h) in place of the reference's offline step
(scannet/compute_normal_for_pc.py:29-48, ARKitScenes/dataset/compute_normal_for_pc.py:25-38: MeshLab's
`compute_normals_for_point_sets` with k = 100, smoothiter = 5, flipflag = True, viewpos = pc_center, then a flip towards
(p - pc_center) . n >= 0):

    normals = estimate_normals(xyz)                         # (B, N, 3) f32 on the GPU -> (B, N, 3) f32

The four stages -- k nearest neighbours, plane fit over them, sign-aligned neighbour averaging, viewpoint flip -- are this
project's contract (the header states every operation); agreement with MeshLab's own output has NOT been checked, MeshLab is
not available to this project.  The final orientation does not depend on it.  Clouds with non-finite coordinates are not
supported and nothing reads back to check.  There is no CPU path.
"""
import torch

from pointnet2 import _ext

RECIPE_K, RECIPE_SMOOTH_ITERS = 100, 5                    # compute_normal_for_pc.py:40


def recipe_view_centre(xyz):
    """(B, N, 3) -> (B, 3) float64: (mean x, mean y, (max z + mean z) / 2), compute_normal_for_pc.py:34-35.  Torch ops on the
    tensor's device, no host read."""
    p = xyz.detach()[..., :3].to(torch.float64)
    centre = p.mean(dim=1)
    centre[:, 2] = (p[:, :, 2].amax(dim=1) + centre[:, 2]) / 2
    return centre.contiguous()


def estimate_normals(xyz, k=RECIPE_K, smooth_iters=RECIPE_SMOOTH_ITERS, centre=None, cell=None, out=None):
    """xyz (B, N, 3) float32 on the GPU -> normals (B, N, 3) float32, unit length, (p - centre) . n >= 0.
    centre: (B, 3) float64 device tensor; None: recipe_view_centre(xyz).  cell: edge of the k-NN grid's cells, which changes
    the time and never the result; None: _ext.default_knn_cell of the bounding box, which reads six numbers back
    from the device -- pass a cell (SceneBank takes it from the host arrays) where no host read is wanted."""
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError("estimate_normals: xyz must be (B, N, 3)")
    if not 1 <= int(k) <= _ext.KNN_MAX_K:
        raise ValueError(f"estimate_normals: k must be in [1, {_ext.KNN_MAX_K}]")
    if int(smooth_iters) < 0:
        raise ValueError("estimate_normals: smooth_iters must not be negative")
    xyz = xyz.detach().float().contiguous()
    if centre is None:
        centre = recipe_view_centre(xyz)
    centre = centre.to(device=xyz.device, dtype=torch.float64).contiguous()
    if cell is None:
        if xyz.shape[1] == 0 or xyz.shape[0] == 0:
            cell = 1.0
        else:
            box = torch.stack([xyz.amin(dim=(0, 1)), xyz.amax(dim=(0, 1))]).cpu()
            cell = _ext.default_knn_cell(box[0].tolist(), box[1].tolist(), xyz.shape[1], k)
    return _ext.estimate_normals(xyz, centre, int(k), int(smooth_iters), float(cell), out=out)
