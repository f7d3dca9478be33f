"""The whole semi-supervised objective of Omni-PQ as ONE criterion: the reference's train.py:496-543

    total_loss = loss + consistency_loss + gamma_mixture_filter_loss + arkit_pc_loss

restated with this repository's four term functions, none of which reads the device from the host -- so the objective can be
the criterion of `train_step.CapturedStep(teacher=..., teacher_to_criterion=True)`:

    objective = SemiSupervisedObjective(DATASET_CONFIG, config)
    stepper = CapturedStep(net, objective, example_inputs, example_labels, teacher=ema_net, teacher_to_criterion=True)
    loss = stepper.step(inputs, labels)              # objective.stats: every reported term, detached device scalars

The batch is the labelled scenes followed by the unlabelled ones (train.py:480-485), `labels` one flat dict of device tensors
(as CapturedStep clones it):

    <key>                  the labelled batch's tensors, as the reference's loader names them     (Bl, ...)
    unlabeled.<key>        the unlabelled batch's tensors                                          (Bu, ...)
    consistency_weight     0-dim float32: get_current_consistency_weight(epoch) (train.py:441-454), filled by the host per epoch

What runs, driven by `config` (the reference's command-line flags):

    1. get_loss(first Bl scenes of end_points + the labelled tensors, DATASET_CONFIG, pc_loss=config.pc_loss)     always
       Only tensors of end_points whose leading dimension is Bl + Bu are sliced; everything else is passed as it is.
    2. config.gamma_mixture: gamma_mixture_guide_criterion(remaining scenes + the unlabelled tensors), weighted by
       config.lambda_metric_normal / _vertical / _size / _score
    3. config.ema: `flip_x_axis`, `flip_y_axis`, `rot_mat`, `scale` of both batches concatenated into end_points, then
       get_consistency_loss(end_points, teacher_end_points, DATASET_CONFIG) on the whole batch, times consistency_weight
    4. config.arkit: get_arkit_pc_loss(end_points, unlabelled tensors, DATASET_CONFIG) times config.lambda_arkit_pc_loss

`stats` also holds the supervised terms, which the reference loses with its `gt_end_points`.
"""
import torch

from loss_helper_pq import get_loss
from models.utils.arkit_loss_util import get_arkit_pc_loss
from models.utils.gamma_mixture_loss_util import gamma_mixture_guide_criterion
from models.utils.mean_teacher_consistency_util import get_consistency_loss

UNLABELED = "unlabeled."
WEIGHT_KEY = "consistency_weight"
AUGMENTATION_KEYS = ("flip_x_axis", "flip_y_axis", "rot_mat", "scale")           # train.py:526
SUPERVISED_STATS = ("loss", "vote_loss", "objectness_loss", "box_loss", "sem_cls_loss_sum", "quad_score_loss_sum",
                    "quad_center_loss_sum", "quad_vector_loss_sum", "quad_size_loss_sum", "quad_loss_sum",
                    "physical_constraints_loss", "collisions")
METRICS = ("metric_normal", "metric_vertical", "metric_size", "metric_score")
BATCH_ANCHORS = ("last_quad_center", "last_center")       # a prediction whose leading dimension is the whole batch


def _leading(tensors, what):
    for key in ("center_label", "point_clouds"):
        if key in tensors:
            return int(tensors[key].shape[0])
    for t in tensors.values():
        if torch.is_tensor(t) and t.dim() >= 1:
            return int(t.shape[0])
    raise ValueError(f"SemiSupervisedObjective: no {what} tensor in `labels` to take the batch size from")


class SemiSupervisedObjective:
    """criterion(end_points, labels, teacher_end_points=None) -> the total loss; see the module docstring.

    DATASET_CONFIG   what get_loss and the consistency loss read (class counts, mean_size_arr)
    config           pc_loss, gamma_mixture, ema, arkit (switches); lambda_metric_normal / _vertical / _size / _score and
                     lambda_arkit_pc_loss (read only when their term is on)
    CONFIG_DICT      handed to the guide criterion, which ignores it as the reference's does outside its dumping code"""

    def __init__(self, DATASET_CONFIG, config, CONFIG_DICT=None):
        self.DATASET_CONFIG, self.config, self.CONFIG_DICT = DATASET_CONFIG, config, CONFIG_DICT
        self.stats = {}

    @staticmethod
    def split_labels(labels):
        """-> (labelled tensors, unlabelled tensors without their prefix, consistency_weight or None)"""
        labelled = {k: v for k, v in labels.items() if not k.startswith(UNLABELED) and k != WEIGHT_KEY}
        unlabelled = {k[len(UNLABELED):]: v for k, v in labels.items() if k.startswith(UNLABELED)}
        return labelled, unlabelled, labels.get(WEIGHT_KEY)

    def __call__(self, end_points, labels, teacher_end_points=None):
        cfg = self.config
        labelled, unlabelled, weight = self.split_labels(labels)
        Bl = _leading(labelled, "labelled")
        Bu = _leading(unlabelled, "unlabelled") if unlabelled else 0
        anchor = next((end_points[k] for k in BATCH_ANCHORS if k in end_points), None)
        if anchor is None:
            raise ValueError(f"SemiSupervisedObjective: end_points holds none of {BATCH_ANCHORS}")
        Bt, dev = int(anchor.shape[0]), anchor.device
        if Bt != Bl + Bu:
            raise ValueError(f"SemiSupervisedObjective: end_points holds {Bt} scenes, the labels {Bl} labelled + {Bu} unlabelled")

        def part(lo, hi, extra):
            out = {k: (v[lo:hi] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == Bt else v) for k, v in end_points.items()}
            for k, v in extra.items():
                if k in out:
                    raise ValueError(f"SemiSupervisedObjective: `{k}` is both a label and an output of the model")   # :501
                out[k] = v
            return out

        def scalar(v):
            if torch.is_tensor(v):
                return v.detach().float().reshape(())
            return torch.full((), float(v), device=dev, dtype=torch.float32)

        stats = {}
        # 1. the detector's ground-truth loss on the labelled scenes
        loss, gt_end_points = get_loss(part(0, Bl, labelled), self.DATASET_CONFIG, pc_loss=cfg.pc_loss)
        for k in SUPERVISED_STATS:
            if k in gt_end_points:
                stats[k] = scalar(gt_end_points[k])
        # 2. the gamma-mixture guide on the unlabelled scenes
        metrics, filter_loss = (0.0, 0.0, 0.0, 0.0), 0.0
        if cfg.gamma_mixture:
            metrics = gamma_mixture_guide_criterion(part(Bl, Bt, unlabelled), self.DATASET_CONFIG, config=cfg,
                                                    CONFIG_DICT=self.CONFIG_DICT)
            filter_loss = cfg.lambda_metric_normal * metrics[0] + cfg.lambda_metric_vertical * metrics[1] \
                + cfg.lambda_metric_size * metrics[2] + cfg.lambda_metric_score * metrics[3]
        # 3. the mean-teacher consistency on the whole batch
        consistency_loss = 0.0
        if cfg.ema:
            if teacher_end_points is None or weight is None:
                raise ValueError("SemiSupervisedObjective: config.ema needs the teacher's end_points (CapturedStep(teacher=..., "
                                 f"teacher_to_criterion=True)) and labels['{WEIGHT_KEY}']")
            for key in AUGMENTATION_KEYS:
                end_points[key] = torch.cat([labelled[key], unlabelled[key]], dim=0)
            consistency_loss, end_points = get_consistency_loss(end_points, teacher_end_points, self.DATASET_CONFIG)
            consistency_loss = consistency_loss * weight
        # 4. the unlabelled scenes' boxes against their predicted quads
        arkit_pc_loss, collisions = 0.0, 0
        if cfg.arkit:
            arkit_pc_loss, collisions = get_arkit_pc_loss(end_points, unlabelled, self.DATASET_CONFIG)
            arkit_pc_loss = arkit_pc_loss * cfg.lambda_arkit_pc_loss
        total_loss = loss + consistency_loss + filter_loss + arkit_pc_loss                                             # :543
        for k, v in zip(METRICS, metrics):
            stats[k] = scalar(v)
        stats.update(gamma_mixture_filter_loss=scalar(filter_loss), consistency_loss=scalar(consistency_loss),
                     arkit_pc_loss=scalar(arkit_pc_loss), arkit_collisions=scalar(collisions), total_loss=scalar(total_loss))
        self.stats = stats
        return total_loss
