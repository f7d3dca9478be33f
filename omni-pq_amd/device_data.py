"""Device-resident scenes: a batch of training items sampled, augmented and labelled by csrc/batch_assemble.hip
(include/omnipq_data.h states the arithmetic) instead of by the datasets' `__getitem__` on the host
(scannet/scannet_detection_dataset.py:86-312, ARKitScenes/arkitscenes_dataset.py:83-233).

    bank = SceneBank("cuda", DATASET_CONFIG, use_height=True)
    for name in scan_names:                                  # once: file reading and get_quads stay with the caller
        bank.add_scene(name, vertices, normals, instance_labels, semantic_labels, boxes, *get_quads(name))
    train_loader = DeviceLoader(bank, batch_size=8, seed=0, rank=rank, world_size=world, net=model)
    for epoch in ...:
        train_loader.sampler.set_epoch(epoch)
        for batch_idx, batch_data_label in enumerate(train_loader):      # train.py:465: the tensors are already resident

What is static per scene is computed at registration with the reference's expressions (floor height and height column,
colour normalisation, dense instance ids, class index of every box, the ARKit box preparation); what depends on the draw and on
the four augmentation numbers runs on the device, four launches per batch (two for the unlabelled flavour), no host read.
There is no CPU path: `assemble` raises without the library and a GPU.
"""
import ctypes

import numpy as np
import torch

from pointnet2 import _ext

_lib = _ext._lib

MAX_NUM_OBJ, MAX_NUM_QUAD, MAX_NUM_HQUAD, NUM_PROPOSAL, MAX_INSTANCES, META_INTS, LABEL_DOUBLES, PARAM_DOUBLES = (
    _ext.const("OMNIPQ_ASM_" + name) for name in ("MAX_OBJ", "MAX_QUAD", "MAX_HQUAD", "NUM_PROPOSAL", "MAX_INSTANCES",
                                                  "META_INTS", "LABEL_DOUBLES", "PARAM_DOUBLES"))
MEAN_COLOR_RGB = np.array([109.8, 97.2, 83.8])              # scannet_detection_dataset.py:34

_Bank = _ext.struct("omnipq_asm_bank")
_Batch = _ext.struct("omnipq_asm_batch")
_Out = _ext.struct("omnipq_asm_out")

# the arrays of omnipq_asm_out: (key, trailing shape, dtype, flavours that carry it)
_f32, _i64, _i32 = torch.float32, torch.int64, torch.int32
OUT_FIELDS = (("point_clouds", ("k", "pitch"), _f32, (0, 1)), ("vertex_normals", ("k", 3), _f32, (0, 1)),
              ("ema_point_clouds", ("k", "pitch"), _f32, (0, 1)), ("choices", ("k",), _i32, (0, 1)),
              ("ema_choices", ("k",), _i32, (0, 1)), ("semantic_labels", ("k",), _f32, (0,)),
              ("pcl_color", ("k", 3), _f32, (0,)), ("vote_label", ("k", 9), _f32, (0,)),
              ("vote_label_mask", ("k",), _i64, (0,)), ("point_instance_label", ("k",), _i64, (0,)),
              ("center_label", (MAX_NUM_OBJ, 3), _f32, (0, 1)), ("heading_class_label", (MAX_NUM_OBJ,), _i64, (0, 1)),
              ("heading_residual_label", (MAX_NUM_OBJ,), _f32, (0, 1)), ("size_class_label", (MAX_NUM_OBJ,), _i64, (0,)),
              ("size_residual_label", (MAX_NUM_OBJ, 3), _f32, (0,)), ("size_gts", (MAX_NUM_OBJ, 3), _f32, (0,)),
              ("size_label", (MAX_NUM_OBJ, 3), _f32, (1,)), ("sem_cls_label", (MAX_NUM_OBJ,), _i64, (0,)),
              ("box_label_mask", (MAX_NUM_OBJ,), _f32, (0,)), ("num_gt_boxes", (NUM_PROPOSAL,), _i64, (0, 1)),
              ("gt_quad_centers", (MAX_NUM_QUAD, 3), _f32, (0,)), ("gt_normal_vectors", (MAX_NUM_QUAD, 3), _f32, (0,)),
              ("gt_quad_sizes", (MAX_NUM_QUAD, 2), _f32, (0,)), ("num_gt_quads", (NUM_PROPOSAL,), _i64, (0,)),
              ("num_total_quads", (NUM_PROPOSAL,), _i64, (0,)), ("horizontal_quads", (4, 4, 3), _f32, (0,)),
              ("flip_x_axis", (), _i64, (0, 1)), ("flip_y_axis", (), _i64, (0, 1)), ("rot_mat", (3, 3), _f32, (0, 1)),
              ("scale", (), _f32, (0, 1)), ("scan_idx", (), _i64, (0,)))
# `choices` / `ema_choices` are extensions (the rows drawn); everything else is a key of the reference's item

if sorted(f[0] for f in OUT_FIELDS) != sorted(name for name, _ in _Out._fields_):
    raise ImportError("device_data: OUT_FIELDS and the loaded library's omnipq_asm_out name different arrays")


def rotz(t):
    """utils/pc_util.py:312-318"""
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def pack_params(params):
    """[(flip_x, flip_y, rot_mat (3, 3) float64, scale)] -> (b, 12) float64, the layout of omnipq_asm_batch.params"""
    out = np.zeros((len(params), PARAM_DOUBLES), np.float64)
    for i, (fx, fy, rot, scale) in enumerate(params):
        rot = np.asarray(rot, np.float64)
        if rot.shape != (3, 3):
            raise ValueError("params: rot_mat must be (3, 3)")
        out[i, 0], out[i, 1], out[i, 2:11], out[i, 11] = bool(fx), bool(fy), rot.reshape(9), float(scale)
    return out


def _align_boxes(points, boxes):
    """Oriented boxes (nb, 7) -> the axis-aligned boxes the ARKit item labels with (arkitscenes_dataset.py:102-126), float64:
    the scene turns by the median box heading folded into a quarter turn; the origin moves to the median x / y of the points
    in the middle 70 % of the height range and to the 5th height percentile; a box whose remaining heading lies within 45
    degrees of the y axis swaps its two horizontal sizes.  The points themselves stay as they are (:104, :115)."""
    out = boxes.copy()
    turn = np.percentile(out[:, 6] % (np.pi / 2), 50)
    z = points[:, 2]
    band = (z >= np.percentile(z, 15)) & (z <= np.percentile(z, 85))
    origin = np.array([np.percentile(points[band, 0], 50), np.percentile(points[band, 1], 50), np.percentile(z, 5)])
    out[:, :3] = np.dot(out[:, :3], rotz(turn).T) - origin
    heading = (out[:, 6] - turn) % (2 * np.pi)
    eighth = np.pi / 4
    swapped = ((eighth <= heading) & (heading <= eighth * 3)) | ((eighth * 5 <= heading) & (heading <= eighth * 7))
    out[:, 3], out[:, 4] = np.where(swapped, boxes[:, 4], boxes[:, 3]), np.where(swapped, boxes[:, 3], boxes[:, 4])
    out[:, 6] = heading
    return out


IDENTITY = (False, False, np.identity(3), 1.0)


class SceneBank:
    """Scenes of ONE flavour (labelled ScanNet items via add_scene, or unlabelled ARKit items via add_unlabelled_scene) in one
    packed device arena with a per-scene offset / row-count table.  Scenes are staged on the host as they are added and
    uploaded together by the first `assemble` (or `upload()`); adding a scene later uploads again."""

    def __init__(self, device, dataset_config=None, use_height=True, use_color=False, max_bytes=64 << 30, seed=0):
        self.device = torch.device(device)
        self.config = dataset_config
        self.use_height, self.use_color, self.max_bytes = bool(use_height), bool(use_color), int(max_bytes)
        self.flavour = None
        self.names = []
        self._rows = []                  # per scene: dict of host arrays
        self.bytes = 0
        self._dev = None
        self._seed_value = int(seed)
        self._seed = None
        self._rng = np.random.RandomState(seed)

    # ---- registration (host only) ---------------------------------------------------------------------------------------
    def _admit(self, name, flavour, host):
        if self.flavour not in (None, flavour):
            raise ValueError(f"SceneBank: {name}: a bank holds labelled or unlabelled scenes, not both")
        n = host["points"].shape[0]
        if n < 1:
            raise ValueError(f"SceneBank: {name}: a scene needs at least one point")
        size = sum(v.nbytes for v in host.values() if isinstance(v, np.ndarray))
        if self.bytes + size > self.max_bytes:
            raise ValueError(f"SceneBank: {name}: {self.bytes + size} bytes exceed max_bytes = {self.max_bytes}")
        self.flavour = flavour
        self.bytes += size
        self.names.append(name)
        self._rows.append(host)
        self._dev = None
        return len(self.names) - 1

    def add_scene(self, name, vertices, normals=None, instance_labels=None, semantic_labels=None, boxes=None, rectangles=None,
                  total_quad_num=None, horizontal_quads=None):
        """vertices (n, 6) xyz + rgb (or (n, 3) without use_color), normals (n, 3), instance_labels, semantic_labels (n),
        boxes (nb, 7) centre, size, nyu40 id (`_bbox.npy`), and what get_quads(name) returns.  -> the scene's slot.
        normals=None: the scene has no `.normal.npy`; they are estimated on the device at upload with the constants of
        scannet/compute_normal_for_pc.py (point_normals.estimate_normals) and stand in the arena where given ones would.
        Only `normals` may be left out (the defaults of the arguments behind it keep the positional order of old calls).
        The arena is float32: vertices and normals are taken as the float32 arrays the dataset's files hold (the bit-for-bit
        agreement with the reference's item is for such files; a float64 file would be rounded here, not after the rotation)."""
        if self.config is None:
            raise ValueError("SceneBank: labelled scenes need a dataset_config (nyu40ids, mean_size_arr)")
        if any(v is None for v in (instance_labels, semantic_labels, boxes, rectangles, total_quad_num, horizontal_quads)):
            raise TypeError("SceneBank.add_scene: only `normals` may be left out")
        mesh_vertices = np.array(vertices, np.float32)
        n = mesh_vertices.shape[0]
        estimate = normals is None
        if estimate:
            normals = np.zeros((n, 3), np.float32)           # the arena's rows; filled by upload()
        boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
        rectangles = np.asarray(rectangles, np.float64)
        rectangles = rectangles.reshape(-1, rectangles.shape[-1] if rectangles.ndim == 2 else 8)
        horizontal_quads = np.asarray(horizontal_quads, np.float64).reshape(-1, 4, 3)
        if boxes.shape[0] > MAX_NUM_OBJ:
            raise ValueError(f"SceneBank: {name}: {boxes.shape[0]} boxes, the item holds {MAX_NUM_OBJ}")
        if rectangles.shape[0] > MAX_NUM_QUAD:
            raise ValueError(f"SceneBank: {name}: {rectangles.shape[0]} rectangles, the item holds {MAX_NUM_QUAD}")
        if horizontal_quads.shape[0] > MAX_NUM_HQUAD:
            raise ValueError(f"SceneBank: {name}: {horizontal_quads.shape[0]} horizontal quads, the item holds {MAX_NUM_HQUAD}")
        uniq, dense = np.unique(np.asarray(instance_labels).reshape(-1), return_inverse=True)
        if len(uniq) > MAX_INSTANCES:
            raise ValueError(f"SceneBank: {name}: {len(uniq)} instances, the extent table holds {MAX_INSTANCES}")
        if rectangles.shape[0] and rectangles.shape[1] < 8:
            raise ValueError(f"SceneBank: {name}: rectangles need 8 columns (centre, normal, size)")
        if not (len(dense) == n == np.asarray(semantic_labels).reshape(-1).shape[0] == np.asarray(normals).shape[0]):
            raise ValueError(f"SceneBank: {name}: vertices, normals and labels differ in length")
        # :112-122
        if not self.use_color:
            point_cloud = mesh_vertices[:, 0:3]
            colors = mesh_vertices[:, 3:6] if mesh_vertices.shape[1] >= 6 else np.zeros((n, 3), np.float32)
        else:
            point_cloud = mesh_vertices[:, 0:6]
            point_cloud[:, 3:] = (point_cloud[:, 3:] - MEAN_COLOR_RGB) / 256.0
            colors = None
        if self.use_height:
            floor_height = np.percentile(point_cloud[:, 2], 0.99)
            height = point_cloud[:, 2] - floor_height
            point_cloud = np.concatenate([point_cloud, np.expand_dims(height, 1)], 1)
        ids = np.asarray(self.config.nyu40ids)
        cls = np.zeros(boxes.shape[0])
        for j, x in enumerate(boxes[:, -1]):                # :248
            where = np.where(ids == x)[0]
            if where.size == 0:
                raise ValueError(f"SceneBank: {name}: box {j} has class id {x}, which is not in nyu40ids")
            cls[j] = where[0]
        labels = np.zeros(LABEL_DOUBLES)
        bx = labels[:MAX_NUM_OBJ * 7].reshape(MAX_NUM_OBJ, 7)
        bx[:boxes.shape[0], 0:6], bx[:boxes.shape[0], 6] = boxes[:, 0:6], cls
        labels[MAX_NUM_OBJ * 7:MAX_NUM_OBJ * 7 + MAX_NUM_QUAD * 8].reshape(MAX_NUM_QUAD, 8)[:rectangles.shape[0]] = rectangles[:, 0:8]
        labels[MAX_NUM_OBJ * 7 + MAX_NUM_QUAD * 8:].reshape(4, 4, 3)[:horizontal_quads.shape[0]] = horizontal_quads
        host = {"points": np.ascontiguousarray(point_cloud, np.float32), "normals": np.ascontiguousarray(normals, np.float32),
                "instance": dense.astype(np.int32), "semantic": np.asarray(semantic_labels).reshape(-1).astype(np.int32),
                "labels": labels, "meta": np.array([n, len(uniq), boxes.shape[0], rectangles.shape[0], int(total_quad_num),
                                                    horizontal_quads.shape[0], 0, 0], np.int32)}
        if colors is not None:
            host["colors"] = np.ascontiguousarray(colors, np.float32)
        host["estimate_normals"] = estimate
        return self._admit(name, 0, host)

    def add_unlabelled_scene(self, name, vertices, normals=None, boxes=None):
        """The ARKit item: vertices (n, 3), normals (n, 3), boxes (nb, 7) centre, size, heading as `_bbox.npy` holds them.
        The static box preparation of arkitscenes_dataset.py:102-131 runs here, once (`_align_boxes`).  float32 points and
        normals are assumed, as the dataset's files hold them.  normals=None: estimated on the device at upload, as in
        add_scene (ARKitScenes/dataset/compute_normal_for_pc.py has the same constants)."""
        if boxes is None:
            raise TypeError("SceneBank.add_unlabelled_scene: only `normals` may be left out")
        points = np.array(vertices, np.float32)[:, 0:3]
        estimate = normals is None
        if estimate:
            normals = np.zeros((points.shape[0], 3), np.float32)
        bb = np.array(boxes, np.float64).reshape(-1, 7)
        if bb.shape[0] > MAX_NUM_OBJ:
            raise ValueError(f"SceneBank: {name}: {bb.shape[0]} boxes, the item holds {MAX_NUM_OBJ}")
        if points.shape[0] != np.asarray(normals).shape[0]:
            raise ValueError(f"SceneBank: {name}: vertices and normals differ in length")
        if bb.shape[0]:
            bb = _align_boxes(points, bb)
        mesh_vertices = points
        labels = np.zeros(LABEL_DOUBLES)
        labels[:MAX_NUM_OBJ * 7].reshape(MAX_NUM_OBJ, 7)[:bb.shape[0], 0:6] = bb[:, 0:6]
        n = mesh_vertices.shape[0]
        host = {"points": np.ascontiguousarray(mesh_vertices), "normals": np.ascontiguousarray(normals, np.float32),
                "labels": labels, "meta": np.array([n, 0, bb.shape[0], 0, 0, 0, 0, 0], np.int32), "estimate_normals": estimate}
        return self._admit(name, 1, host)

    def __len__(self):
        return len(self.names)

    @property
    def pitch(self):
        return 3 + (3 if self.use_color and self.flavour == 0 else 0) + (1 if self.use_height and self.flavour == 0 else 0)

    # ---- the device side --------------------------------------------------------------------------------------------------
    def upload(self):
        """-> dict of the arena's device tensors (uploaded once; the kernels only read them)"""
        if self._dev is not None:
            return self._dev
        if not self._rows:
            raise ValueError("SceneBank: no scene has been added")
        if self.device.type != "cuda":
            raise RuntimeError("SceneBank: CPU not supported (the HIP path has no CPU fallback)")

        def cat(key):
            if key not in self._rows[0]:
                return None
            return torch.from_numpy(np.concatenate([r[key] for r in self._rows])).to(self.device)

        counts = np.array([r["points"].shape[0] for r in self._rows], np.int64)
        dev = {k: cat(k) for k in ("points", "normals", "colors", "instance", "semantic")}
        dev["row_offset"] = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)).to(self.device)
        dev["meta"] = torch.from_numpy(np.stack([r["meta"] for r in self._rows])).to(self.device)
        dev["labels"] = torch.from_numpy(np.stack([r["labels"] for r in self._rows])).to(self.device)
        dev["rows_total"] = int(counts.sum())
        self._estimate_missing_normals(dev, counts)
        if self.flavour == 0:
            dev["nyu40ids"] = torch.tensor(np.asarray(self.config.nyu40ids).astype(np.int32), device=self.device)
            dev["mean_size"] = torch.tensor(np.asarray(self.config.mean_size_arr, np.float64), device=self.device)
        if self._seed is None:
            self._seed = torch.tensor([self._seed_value], dtype=torch.int64, device=self.device)
        self._dev = dev
        return dev

    def _estimate_missing_normals(self, dev, counts):
        """Scenes registered without normals: the recipe of compute_normal_for_pc.py:34-47 on the uploaded float32 coordinates
        (k = 100, 5 smoothing steps, the recipe's view centre), written into the arena's rows.  The grid's cell comes from the
        host copy of the points: nothing is read back from the device."""
        if not any(r["estimate_normals"] for r in self._rows):
            return
        import point_normals
        first = 0
        for r, n in zip(self._rows, counts.tolist()):
            if r["estimate_normals"]:
                xyz = dev["points"][first:first + n, 0:3].contiguous().unsqueeze(0)
                host_xyz = r["points"][:, 0:3]
                cell = _ext.default_knn_cell(host_xyz.min(0), host_xyz.max(0), n, point_normals.RECIPE_K)
                point_normals.estimate_normals(xyz, cell=cell, out=dev["normals"][first:first + n].unsqueeze(0))
            first += n

    @property
    def seed(self):
        """(1,) int64 device tensor: the word the draw hashes.  The bank's own: not the dropout counter.  The same value
        gives the same draws; advance it (`bank.seed.add_(1)`, capturable) between two batches that must differ."""
        self.upload()
        return self._seed

    def draw_params(self, b, augment=True):
        """The four numbers per item of :164-204, from the bank's own host generator -> [(flip_x, flip_y, rot_mat, scale)]"""
        if not augment:
            return [IDENTITY] * b
        out = []
        for _ in range(b):
            fx = self._rng.random_sample() > 0.5
            fy = self._rng.random_sample() > 0.5
            rot_angle = (self._rng.random_sample() * np.pi / 18) - np.pi / 36
            rot_angle += int(self._rng.randint(4)) * np.pi / 2
            out.append((bool(fx), bool(fy), rotz(rot_angle), self._rng.random_sample() * 0.3 + 0.85))
        return out

    def make_buffers(self, b, num_points=40000):
        """Static tensors for `assemble(out=...)`: every output key of the flavour plus the workspace."""
        if self.flavour is None:
            raise ValueError("SceneBank: no scene has been added")
        dims = {"k": int(num_points), "pitch": self.pitch}
        out = {}
        for key, shape, dtype, flavours in OUT_FIELDS:
            if self.flavour in flavours:
                out[key] = torch.empty((b,) + tuple(dims.get(s, s) for s in shape), dtype=dtype, device=self.device)
        if self.flavour == 0:
            out["use_gt"] = torch.ones((b,), dtype=torch.bool, device=self.device)          # :277 with start_proportion 0
            if self.use_color:
                del out["pcl_color"]                         # :112-117: the item carries no separate colours then
        out["_workspace"] = torch.empty((max(int(_lib.omnipq_assemble_workspace_bytes(b)), 8),), dtype=torch.uint8,
                                        device=self.device)
        return out

    def assemble(self, slots, params=None, choices=None, ema_choices=None, num_points=40000, augment=True, out=None):
        """-> the collated batch of the items of `slots`: the reference item's keys, dtypes and shapes with a leading batch
        dimension (`scan_name`: a list), plus `choices` / `ema_choices` (B, num_points) int32, the rows drawn.

        slots: a sequence of scene slots, or a (B,) int32 device tensor (then `scan_name` is left out: no host read).
        params: [(flip_x, flip_y, rot_mat float64, scale)] per item, or a (B, 12) float64 device tensor in the layout of
        `pack_params`; None: drawn on the host (`draw_params`), identity when augment is False.
        choices / ema_choices: (B, num_points) int32 device tensors to use instead of the device draw.
        out: the dict `make_buffers` returned: the launches write into it and allocate nothing."""
        dev = self.upload()
        on_device = torch.is_tensor(slots) and slots.is_cuda
        b = int(slots.shape[0]) if torch.is_tensor(slots) else len(slots)
        k = int(num_points)
        if on_device:
            if slots.dtype != torch.int32 or not slots.is_contiguous():
                raise ValueError("assemble: device slots must be a contiguous int32 tensor")
            slots_dev = slots
        else:
            host_slots = [int(s) for s in slots]
            if any(s < 0 or s >= len(self) for s in host_slots):
                raise ValueError("assemble: a slot outside the bank")
            slots_dev = torch.tensor(host_slots, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        if torch.is_tensor(params):
            if not (params.is_cuda and params.dtype == torch.float64 and tuple(params.shape) == (b, PARAM_DOUBLES) and
                    params.is_contiguous()):
                raise ValueError("assemble: device params must be a contiguous (B, 12) float64 tensor")
            params_dev = params
        else:
            if params is None:
                params = self.draw_params(b, augment)
            if len(params) != b:
                raise ValueError("assemble: one parameter tuple per item")
            params_dev = torch.from_numpy(pack_params(params)).pin_memory().to(self.device, non_blocking=True)
        for name, t in (("choices", choices), ("ema_choices", ema_choices)):
            if t is not None and not (t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (b, k) and t.is_contiguous()):
                raise ValueError(f"assemble: {name} must be a contiguous (B, num_points) int32 device tensor")
        if out is None:
            out = self.make_buffers(b, k)
        want = {key: ((b,) + tuple({"k": k, "pitch": self.pitch}.get(s, s) for s in shape), dtype)
                for key, shape, dtype, flavours in OUT_FIELDS if self.flavour in flavours and key in out}
        missing = [key for key, _, _, flavours in OUT_FIELDS
                   if self.flavour in flavours and key not in out and key != "pcl_color"]
        if missing:
            raise ValueError(f"assemble: out lacks {missing} (make_buffers)")
        for key, (shape, dtype) in want.items():
            t = out[key]
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != slots_dev.device:
                raise ValueError(f"assemble: out[{key!r}] must be a contiguous {shape} {dtype} tensor on the bank's device")
        if b == 0:
            return {key: v for key, v in out.items() if not key.startswith("_")}

        bank = _Bank(len(self), self.pitch, (self.pitch - 1) if (self.use_height and self.flavour == 0) else -1,
                     dev["rows_total"], *[dev[n].data_ptr() if dev.get(n) is not None else None
                                          for n in ("points", "normals", "colors", "instance", "semantic", "row_offset",
                                                    "meta", "labels")])
        ids, sizes = dev.get("nyu40ids"), dev.get("mean_size")
        batch = _Batch(b, k, self.flavour, 0 if ids is None else ids.numel(), 0 if sizes is None else sizes.shape[0],
                       slots_dev.data_ptr(), params_dev.data_ptr(), self._seed.data_ptr(),
                       None if choices is None else choices.data_ptr(), None if ema_choices is None else ema_choices.data_ptr(),
                       None if ids is None else ids.data_ptr(), None if sizes is None else sizes.data_ptr())
        outs = _Out(**{f[0]: out[f[0]].data_ptr() for f in OUT_FIELDS if f[0] in out})
        ws = out.get("_workspace")
        if ws is None or ws.numel() < int(_lib.omnipq_assemble_workspace_bytes(b)):
            raise ValueError("assemble: out['_workspace'] is missing or too small (make_buffers)")
        _ext._run(_lib.omnipq_assemble_batch, slots_dev, ctypes.byref(bank), ctypes.byref(batch), ctypes.byref(outs),
                  ctypes.c_void_p(ws.data_ptr()))
        # The launches hold raw pointers.  Caller-owned buffers keep what the launches read (a captured graph reads it again
        # on every replay).  Without `out` the slots, parameters and workspace made above are released when this returns: they
        # were allocated on the stream the launches were queued on, and the caching allocator hands a block out again only in
        # that stream's order, behind them.  Supplied `choices` / `ema_choices` must likewise belong to the calling stream.
        out["_inputs"] = (slots_dev, params_dev, choices, ema_choices)
        res = {key: v for key, v in out.items() if not key.startswith("_")}
        if not on_device:
            res["scan_name"] = [self.names[s] for s in host_slots]
        return res


class _Sampler:
    """The `.sampler` of the reference's loader: DistributedSampler's epoch switch (train.py:400)."""

    def __init__(self):
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)


class DeviceLoader:
    """Iterable like the DataLoader of train.py:260-268 over a SceneBank: shuffling, sharding and padding are those of
    torch's DistributedSampler (a permutation of the scenes from `seed + epoch`, padded with its own head to a multiple of
    world_size, every world_size-th element from `rank`), batching is DataLoader's (drop_last).  Every batch is assembled on the
    device; with `net` the sampling prefetch of its `point_clouds` is started (`net.prefetch`, as InputPipeline.push does) when
    the batch is handed out, so the plan the backbone holds is the one of the batch forward() sees next.  The tensors are
    resident: the driver's `.cuda(non_blocking=True)` returns them as they are.  By default the launches go on the consumer's
    stream, one batch at a time, between its steps.  side_stream=True assembles one batch ahead on a stream of the loader's
    own, ordered by events; beside the replayed step that cost more than it returned (profiles/assemble_ab.txt, DESIGN 5.4
    and 10)."""

    def __init__(self, bank, batch_size, shuffle=True, drop_last=True, seed=0, rank=0, world_size=1, net=None,
                 num_points=40000, augment=True, side_stream=False):
        if batch_size < 1 or world_size < 1 or not 0 <= rank < world_size:
            raise ValueError("DeviceLoader: batch_size >= 1 and 0 <= rank < world_size")
        self.bank, self.batch_size, self.shuffle, self.drop_last = bank, int(batch_size), bool(shuffle), bool(drop_last)
        self.seed, self.rank, self.world_size, self.net = int(seed), int(rank), int(world_size), net
        self.num_points, self.augment, self.side_stream = int(num_points), bool(augment), bool(side_stream)
        self.sampler = _Sampler()
        self._stream = None

    @property
    def num_samples(self):
        return -(-len(self.bank) // self.world_size)

    def __len__(self):
        n = self.num_samples
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def epoch_indices(self, epoch=None):
        """this rank's scene slots of the epoch, in order (DistributedSampler.__iter__)"""
        epoch = self.sampler.epoch if epoch is None else int(epoch)
        n = len(self.bank)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + epoch)
            indices = torch.randperm(n, generator=g).tolist()
        else:
            indices = list(range(n))
        total = self.num_samples * self.world_size
        padding = total - len(indices)
        if padding > 0 and indices:
            indices += (indices * (-(-padding // len(indices))))[:padding]
        return indices[self.rank:total:self.world_size]

    def batches(self, epoch=None):
        idx = self.epoch_indices(epoch)
        out = [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]
        if out and self.drop_last and len(out[-1]) < self.batch_size:
            out.pop()
        return out

    def _assemble(self, slots, consumer):
        """assemble one batch -> (batch, event that marks it ready, or None on the consumer's own stream)"""
        if not self.side_stream:
            batch = self.bank.assemble(slots, num_points=self.num_points, augment=self.augment)
            self.bank.seed.add_(1)                           # the next batch draws afresh
            return batch, None
        with torch.cuda.stream(self._stream):
            batch = self.bank.assemble(slots, num_points=self.num_points, augment=self.augment)
            self.bank.seed.add_(1)
            ready = torch.cuda.Event()
            ready.record(self._stream)
        for v in batch.values():                             # allocated on the loader's stream, consumed on the caller's
            if torch.is_tensor(v):
                v.record_stream(consumer)
        return batch, ready

    def _hand_out(self, pending, consumer):
        """The batch becomes the one the consumer runs next: only now is its sampling announced.  The backbone keeps ONE plan,
        keyed on the tensor (Pointnet2Backbone.prefetch): announcing a later batch first would replace it, and forward() would
        sample this one again."""
        batch, ready = pending
        if ready is not None:
            consumer.wait_event(ready)
        if self.net is not None and hasattr(self.net, "prefetch"):
            self.net.prefetch({"point_clouds": batch["point_clouds"]})
        return batch

    def __iter__(self):
        self.bank.upload()
        consumer = torch.cuda.current_stream(self.bank.device)
        if not self.side_stream:                             # nothing to overlap with: one batch at a time, none held back
            for slots in self.batches():
                yield self._hand_out(self._assemble(slots, consumer), consumer)
            return
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.bank.device)
        self._stream.wait_stream(consumer)                   # the arena's upload and the seed word were queued there
        pending = None
        for slots in self.batches():                         # assembled one batch ahead, underneath the consumer's step
            nxt = self._assemble(slots, consumer)
            if pending is not None:
                yield self._hand_out(pending, consumer)
            pending = nxt
        if pending is not None:
            yield self._hand_out(pending, consumer)
