"""semi_objective.SemiSupervisedObjective on the GPU: eager, its total against the four term functions called by hand in the
order of train.py:496-543, bit for bit; and as the criterion of train_step.CapturedStep(teacher=..., teacher_to_criterion=True)
with all four groups on, the replay against the eager stepper.  The host logic alone: tests/test_semi_objective.py."""
import copy
import types

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import loss_inputs
import mt_inputs

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:reduction")]
Bl = Bu = 2
LABEL_KEYS = ("center_label", "heading_class_label", "heading_residual_label", "size_class_label", "size_residual_label",
              "sem_cls_label", "num_gt_boxes", "gt_quad_centers", "gt_normal_vectors", "gt_quad_sizes", "num_gt_quads",
              "vote_label", "vote_label_mask")


def config(arkit=True):
    return types.SimpleNamespace(pc_loss=True, gamma_mixture=True, ema=True, arkit=arkit, lambda_metric_normal=0.5,
                                 lambda_metric_vertical=2.0, lambda_metric_size=0.25, lambda_metric_score=0.125,
                                 lambda_arkit_pc_loss=1.0)


def set_counter(value):
    """the guide criterion's draws follow a device counter of its own: the same start, the same draws"""
    import dropout_state
    from models.utils import gamma_mixture_loss_util as gm
    with dropout_state.STATE.use(gm.SEED_SLOT):
        dropout_state.STATE.set_state("cuda:%d" % torch.cuda.current_device(), value)


def flat_labels(labelled, unlabelled, aug, weight, dev):
    """the flat dict of device tensors the objective reads: labelled keys, `unlabeled.` keys, consistency_weight"""
    out = {k: torch.as_tensor(v).to(dev) for k, v in labelled.items()}
    out.update({"unlabeled." + k: torch.as_tensor(v).to(dev) for k, v in unlabelled.items()})
    for k, v in aug.items():
        out[k], out["unlabeled." + k] = torch.from_numpy(v[:Bl]).to(dev), torch.from_numpy(v[Bl:]).to(dev)
    out["consistency_weight"] = torch.tensor(weight, device=dev)
    return out


def walls(rng, n, room=(6.0, 5.0, 2.6)):
    """n points on the four walls of the room of tests/loss_inputs.py with their inward normals, float32"""
    side = rng.integers(0, 4, n)
    p = rng.uniform((0, 0, 0), room, (n, 3))
    p[:, 0] = np.where(side == 0, 0.0, np.where(side == 1, room[0], p[:, 0]))
    p[:, 1] = np.where(side == 2, 0.0, np.where(side == 3, room[1], p[:, 1]))
    normal = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.float64)[side]
    return (p + 0.01 * rng.standard_normal((n, 3))).astype(np.float32), \
        (normal + 0.05 * rng.standard_normal((n, 3))).astype(np.float32)


def test_the_total_is_the_four_terms_called_by_hand():
    import loss_helper_pq
    import semi_objective
    from models.utils import arkit_loss_util, gamma_mixture_loss_util, mean_teacher_consistency_util
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    lab, pred = loss_inputs.make(41, B=Bl + Bu)
    means = torch.from_numpy(loss_inputs.MEAN_SIZE_ARR.astype(np.float32)).to(dev)

    def outputs(pred, grad):
        ep = {k: torch.from_numpy(v.copy()).to(dev).requires_grad_(grad) for k, v in pred.items()}
        leaves = dict(ep)
        for p in loss_inputs.prefixes():
            ep[p + "size_residuals"] = ep[p + "size_residuals_normalized"] * means[None, None]
        return ep, leaves

    ep, leaves = outputs(pred, True)
    for k in lab:                                                    # what loss_inputs counts as labels but the model outputs
        if k not in LABEL_KEYS:
            ep[k] = torch.from_numpy(lab[k]).to(dev)
    teacher = outputs(loss_inputs.make(42, B=Bl + Bu)[1], False)[0]
    size = loss_inputs.MEAN_SIZE_ARR[lab["size_class_label"]] + lab["size_residual_label"]
    points = [walls(rng, 20000) for _ in range(Bu)]
    unlabelled = {"center_label": lab["center_label"][Bl:], "size_label": size[Bl:].astype(np.float32),
                  "num_gt_boxes": lab["num_gt_boxes"][Bl:], "point_clouds": np.stack([p for p, _ in points]),
                  "vertex_normals": np.stack([n for _, n in points])}
    labels = flat_labels({k: lab[k][:Bl] for k in LABEL_KEYS}, unlabelled, mt_inputs.augmentation(rng, Bl + Bu), 0.3, dev)
    cfg = config()
    names = sorted(leaves)

    objective = semi_objective.SemiSupervisedObjective(loss_inputs.Config, cfg)
    set_counter(777)
    total = objective(dict(ep), labels, teacher)
    grads = torch.autograd.grad(total, [leaves[k] for k in names], allow_unused=True, retain_graph=True)   # (size_residuals)
    stats = objective.stats

    # train.py:496-543 by hand
    labelled, unl, weight = semi_objective.SemiSupervisedObjective.split_labels(labels)
    set_counter(777)
    mine = dict(ep)
    gt = {k: v[:Bl] for k, v in mine.items()}
    gt.update(labelled)
    loss, gt = loss_helper_pq.get_loss(gt, loss_inputs.Config, pc_loss=True)
    guide = {k: v[Bl:] for k, v in mine.items()}
    guide.update(unl)
    metrics = gamma_mixture_loss_util.gamma_mixture_guide_criterion(guide, loss_inputs.Config, config=cfg, CONFIG_DICT=None)
    filter_loss = cfg.lambda_metric_normal * metrics[0] + cfg.lambda_metric_vertical * metrics[1] \
        + cfg.lambda_metric_size * metrics[2] + cfg.lambda_metric_score * metrics[3]
    for key in ("flip_x_axis", "flip_y_axis", "rot_mat", "scale"):
        mine[key] = torch.cat([labelled[key], unl[key]], dim=0)
    consistency, mine = mean_teacher_consistency_util.get_consistency_loss(mine, teacher, loss_inputs.Config)
    consistency = consistency * weight
    arkit, collisions = arkit_loss_util.get_arkit_pc_loss(mine, unl, loss_inputs.Config)
    arkit = arkit * cfg.lambda_arkit_pc_loss
    want = loss + consistency + filter_loss + arkit
    want_grads = torch.autograd.grad(want, [leaves[k] for k in names], allow_unused=True)

    print("terms", {k: float(v) for k, v in stats.items()})
    assert total.dim() == 0 and torch.equal(total.detach(), want.detach()) and bool(torch.isfinite(total))
    for k, v in (("loss", loss), ("consistency_loss", consistency), ("gamma_mixture_filter_loss", filter_loss),
                 ("arkit_pc_loss", arkit), ("arkit_collisions", collisions), ("total_loss", want),
                 ("physical_constraints_loss", gt["physical_constraints_loss"]), ("vote_loss", gt["vote_loss"]),
                 ("metric_vertical", metrics[1])):
        assert stats[k].dim() == 0 and stats[k].dtype == torch.float32 and not stats[k].requires_grad
        assert torch.equal(stats[k], v.detach().float().reshape(())), k
    assert float(stats["loss"]) > 0 and float(stats["consistency_loss"]) > 0 and float(stats["arkit_pc_loss"]) > 0
    assert float(stats["arkit_collisions"]) > 0
    for k, a, b in zip(names, grads, want_grads):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), k
    g = dict(zip(names, grads))
    assert g["last_quad_center"][Bl:].any() and g["last_normal_vector"][Bl:].any()


def test_the_objective_is_the_criterion_of_a_captured_step_with_a_teacher():
    """All four groups on, lambda_arkit_pc_loss = 1, 2 + 2 scenes of 8192 points: the replay equals the eager stepper within
    the bounds of tests/test_gpu_consistency.py::test_criterion_of_a_captured_step_with_a_teacher, the ARKit term is positive,
    and the student's gradients are not those of the objective without it."""
    import bench
    import semi_objective
    import synth
    import train_step
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    pc = synth.make_clouds(80, Bl + Bu, 8192, kind="room")
    mean_size = bench.mean_size_arr()
    labelled = synth.make_labels(pc[:Bl], 81, mean_size_arr=mean_size)
    other = synth.make_labels(pc[Bl:], 82, mean_size_arr=mean_size)
    size = mean_size[other["size_class_label"].numpy()] + other["size_residual_label"].numpy()
    normals = rng.standard_normal((Bu, pc.shape[1], 3))
    unlabelled = {"center_label": other["center_label"], "size_label": size.astype(np.float32),
                  "num_gt_boxes": other["num_gt_boxes"], "point_clouds": pc[Bl:, :, :3].contiguous(),
                  "vertex_normals": (normals / np.linalg.norm(normals, axis=-1, keepdims=True)).astype(np.float32)}
    labels = flat_labels(labelled, unlabelled, mt_inputs.augmentation(rng, Bl + Bu), 0.3, dev)
    pc = pc.to(dev)

    class DatasetConfig(bench.LossConfig):
        mean_size_arr = mean_size

    watch = "decoder.0.linear1.weight"

    def run(graph, arkit):
        net = load_procedural(bench.build_model(0)).to(dev).train()
        zero_dropout(net)
        teacher = copy.deepcopy(net)
        for p in teacher.parameters():
            p.requires_grad_(False)
        objective = semi_objective.SemiSupervisedObjective(DatasetConfig, config(arkit))
        st = train_step.CapturedStep(net, objective, {"point_clouds": pc}, labels, graph=graph, teacher=teacher,
                                     teacher_to_criterion=True)
        assert st.launch == ("hipGraph replay" if graph else "eager")
        set_counter(4242)
        loss = st.step({"point_clouds": pc}, labels)
        torch.cuda.synchronize()
        grad = dict(net.named_parameters())[watch].grad.detach().float().clone()
        return float(loss.detach()), grad, {k: float(v) for k, v in objective.stats.items()}

    def rel(x, y):
        return float((x.double() - y.double()).norm() / (y.double().norm() + 1e-30))

    replay, eager, plain = run(True, True), run(False, True), run(False, False)
    print("replay", replay[0], replay[2], "\neager", eager[0], eager[2], "\nwithout arkit", plain[0])
    print("gradient: replay vs eager", rel(replay[1], eager[1]), "eager vs without arkit", rel(eager[1], plain[1]))
    assert np.isfinite(replay[0]) and replay[2]["arkit_pc_loss"] > 0 and eager[2]["arkit_pc_loss"] > 0
    assert replay[2]["consistency_loss"] > 0 and replay[2]["loss"] > 0
    assert abs(replay[0] - eager[0]) <= 1e-5 * abs(eager[0]), (replay[0], eager[0])
    assert rel(replay[1], eager[1]) <= 3e-2 + 1e-4, rel(replay[1], eager[1])
    assert abs(replay[0] - replay[2]["total_loss"]) <= 1e-6 * abs(replay[0])
    assert plain[2]["arkit_pc_loss"] == 0.0 and plain[2]["arkit_collisions"] == 0.0
    # two eager steps are bit-reproducible (tests/test_train_step.py): what differs here is the ARKit term's gradient
    assert rel(eager[1], plain[1]) > 1e-3, rel(eager[1], plain[1])
