"""Seeded procedural scenes for the device-resident input side (omni-pq_amd/device_data.py, csrc/batch_assemble.hip): the
arrays a ScanNet / ARKit scene consists of on disk (scannet_detection_dataset.py:106-110, :146; arkitscenes_dataset.py:86-88),
small.  Used by tests/golden/make_golden_assemble.py (which serves them to the REFERENCE's `__getitem__`) and by the tests
(which hand the very same arrays to the restatement and to the SceneBank), so the fixture only holds parameters and outputs.

Every scene is a set of point clusters, one per instance id; ids are sparse and unordered on purpose (the bank remaps them).
"""
import numpy as np

from loss_inputs import MEAN_SIZE_ARR

# the 18 NYU40 ids of the ScanNet detection classes (public: VoteNet's model_util_scannet.py)
NYU40IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
OTHER_IDS = np.array([0, 1, 2, 13, 40])            # wall, floor, ... : instances whose points get no vote


class Config:
    """What the dataset's item reads of ScannetDatasetConfig (model_util_scannet.py:28-30); the class mean sizes are the
    synthetic table of tests/loss_inputs.py, not the dataset's file."""
    nyu40ids = NYU40IDS
    nyu40id2class = {int(v): i for i, v in enumerate(NYU40IDS)}
    mean_size_arr = MEAN_SIZE_ARR


#        name    generator seed, rows, sampled, instances, boxes, rectangles, horizontal quads, augment, flips wanted
CASES = {"room": (11, 3000, 1024, 40, 20, 7, 2, True, (True, True)),
         "thin": (12, 700, 1024, 12, 0, 3, 0, True, (False, True)),
         "full": (13, 5000, 2048, 60, 64, 32, 4, True, (True, False)),
         "plain": (11, 3000, 1024, 40, 20, 7, 2, False, (False, False)),
         "arkit": (15, 3000, 1024, 0, 10, 0, 0, True, (True, True))}
LABELLED = ("room", "thin", "full", "plain")


def scene(name):
    """-> dict of the scene's arrays.  Labelled: vertices (n, 6) f32 (xyz, rgb), normals (n, 3) f32, instance_labels,
    semantic_labels (n) int64, boxes (nb, 7) f64 (centre, size, nyu40 id), rectangles (nq, 8) f64, total_quad_num,
    horizontal_quads (nh, 4, 3) f64.  `arkit`: vertices (n, 3) f32, normals, boxes (nb, 7) f64 (centre, size, heading)."""
    gseed, n, _, n_inst, n_box, n_rect, n_h, _, _ = CASES[name]
    rs = np.random.RandomState(gseed)
    f32 = np.float32
    if name == "arkit":
        xyz = (rs.rand(n, 3) * [6.0, 5.0, 2.6] - [3.0, 2.5, 0.2]).astype(f32)
        nrm = rs.randn(n, 3)
        boxes = np.concatenate([rs.rand(n_box, 3) * [6.0, 5.0, 2.0] - [3.0, 2.5, 0.0], 0.3 + rs.rand(n_box, 3),
                                rs.rand(n_box, 1) * 2 * np.pi], 1)
        return {"vertices": xyz, "normals": (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32), "boxes": boxes,
                "types": ["chair"] * n_box}
    # cluster sizes: a long tail, so that some instances draw no point or a single one
    weight = rs.rand(n_inst) ** 4 + 1e-3
    weight[:3] = 3e-4
    owner = rs.choice(n_inst, size=n, p=weight / weight.sum())
    owner[:n_inst] = np.arange(n_inst)                        # every instance exists in the scene
    centre = rs.rand(n_inst, 3) * [6.0, 5.0, 2.0] - [3.0, 2.5, 0.0]
    xyz = (centre[owner] + 0.25 * rs.randn(n, 3)).astype(f32)
    rgb = rs.randint(0, 256, size=(n, 3)).astype(f32)
    nrm = rs.randn(n, 3)
    ids = rs.permutation(200)[:n_inst] * 3 + 1                # sparse instance ids, not in order
    sem_of = np.where(rs.rand(n_inst) < 0.7, rs.choice(NYU40IDS, n_inst), rs.choice(OTHER_IDS, n_inst))
    sem = sem_of[owner]
    # two large instances carry two semantic labels point by point, one inside and one outside the class list: whether
    # their points vote depends on the label of the FIRST sampled point alone (:235-237)
    big = np.argsort(-np.bincount(owner, minlength=n_inst))[:2]
    for g in big:
        rows = np.where(owner == g)[0]
        sem[rows] = np.where(rs.rand(rows.size) < 0.5, NYU40IDS[int(g) % 18], 1)
    order = rs.permutation(n)                                 # rows of an instance are not contiguous
    out = {"vertices": np.concatenate([xyz, rgb], 1)[order], "normals": (nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
           .astype(f32)[order], "instance_labels": ids[owner][order].astype(np.int64), "semantic_labels": sem[order].astype(np.int64)}
    pick = rs.permutation(n_inst)[:n_box] if n_box <= n_inst else rs.randint(0, n_inst, size=n_box)
    out["boxes"] = np.concatenate([centre[pick] + 0.1 * rs.randn(n_box, 3), 0.3 + 1.2 * rs.rand(n_box, 3),
                                   rs.choice(NYU40IDS, n_box)[:, None].astype(np.float64)], 1).reshape(n_box, 7)
    ang = rs.rand(n_rect) * 2 * np.pi
    out["rectangles"] = np.concatenate([rs.rand(n_rect, 3) * [6.0, 5.0, 0.0] + [-3.0, -2.5, 1.3],
                                        np.stack([np.cos(ang), np.sin(ang), np.zeros(n_rect)], 1),
                                        1.0 + 3.0 * rs.rand(n_rect, 1), np.full((n_rect, 1), 2.6)], 1).reshape(n_rect, 8)
    out["total_quad_num"] = n_rect + 2
    out["horizontal_quads"] = (rs.rand(n_h, 4, 3) * [6.0, 5.0, 2.6] - [3.0, 2.5, 0.0]).reshape(n_h, 4, 3)
    return out
