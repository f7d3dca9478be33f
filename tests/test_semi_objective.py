"""The host logic of semi_objective.SemiSupervisedObjective (train.py:496-543 restated) without a GPU: the four term
functions are replaced by recording stubs; checked are the scenes and keys every term receives, the weights, every
combination of the four switches, `stats`, and the refusal of a batch that is not the labelled plus the unlabelled scenes."""
import itertools
import types

import pytest
import torch

Bl, Bu, Q = 2, 3, 4
SUP, CONS, ARK = 7.0, 1.25, 0.5
METRICS = (0.125, 0.25, 0.5, 2.0)


def config(**switches):
    cfg = dict(pc_loss=True, gamma_mixture=True, ema=True, arkit=True, lambda_metric_normal=3.0, lambda_metric_vertical=5.0,
               lambda_metric_size=7.0, lambda_metric_score=11.0, lambda_arkit_pc_loss=0.75)
    cfg.update(switches)
    return types.SimpleNamespace(**cfg)


def batch(Bt=Bl + Bu):
    scene = torch.arange(Bt, dtype=torch.float32)
    ep = {"last_quad_center": scene.reshape(Bt, 1, 1).expand(Bt, Q, 3).clone(), "last_center": scene.reshape(Bt, 1, 1) + 0.5,
          "shared_table": torch.ones(7, 2), "note": "not a tensor"}
    labels = {"center_label": 10.0 + torch.arange(Bl, dtype=torch.float32).reshape(Bl, 1, 1).expand(Bl, 6, 3),
              "unlabeled.center_label": 20.0 + torch.arange(Bu, dtype=torch.float32).reshape(Bu, 1, 1).expand(Bu, 6, 3),
              "unlabeled.point_clouds": torch.zeros(Bu, 8, 3), "consistency_weight": torch.tensor(0.3)}
    for i, key in enumerate(("flip_x_axis", "flip_y_axis", "rot_mat", "scale")):
        labels[key] = torch.full((Bl, 1), float(i))
        labels["unlabeled." + key] = torch.full((Bu, 1), 100.0 + i)
    return ep, labels


@pytest.fixture()
def stubbed(built_lib, monkeypatch):
    import semi_objective
    calls = {}

    def get_loss(end_points, DATASET_CONFIG, pc_loss=True):
        calls["get_loss"] = (dict(end_points), DATASET_CONFIG, pc_loss)
        end_points.update(vote_loss=torch.tensor(1.0), box_loss=torch.tensor(2.0), physical_constraints_loss=0.0, collisions=0,
                          loss=torch.tensor(SUP))
        return end_points["loss"], end_points

    def guide(end_points, DATASET_CONFIG, config=None, CONFIG_DICT=None):
        calls["guide"] = (dict(end_points), DATASET_CONFIG, config, CONFIG_DICT)
        return tuple(torch.tensor(m) for m in METRICS)

    def consistency(end_points, teacher_end_points, DATASET_CONFIG):
        calls["consistency"] = (dict(end_points), teacher_end_points, DATASET_CONFIG)
        return torch.tensor(CONS), end_points

    def arkit(end_points, batch_data_unlabeled, DATASET_CONFIG):
        calls["arkit"] = (dict(end_points), dict(batch_data_unlabeled), DATASET_CONFIG)
        return torch.tensor(ARK), torch.tensor(9.0)

    monkeypatch.setattr(semi_objective, "get_loss", get_loss)
    monkeypatch.setattr(semi_objective, "gamma_mixture_guide_criterion", guide)
    monkeypatch.setattr(semi_objective, "get_consistency_loss", consistency)
    monkeypatch.setattr(semi_objective, "get_arkit_pc_loss", arkit)
    return semi_objective, calls


def test_every_term_receives_its_scenes_and_keys(stubbed):
    semi_objective, calls = stubbed
    ep, labels = batch()
    teacher = {"last_center": torch.zeros(Bl + Bu, 1, 1)}
    dataset, extra = object(), object()
    obj = semi_objective.SemiSupervisedObjective(dataset, config(pc_loss=False), CONFIG_DICT=extra)
    total = obj(ep, labels, teacher)
    # 1. the labelled scenes, the labelled keys, nothing of the unlabelled batch; only full-batch tensors are sliced
    got, cfg, pc_loss = calls["get_loss"]
    assert cfg is dataset and pc_loss is False
    assert torch.equal(got["last_quad_center"][:, 0, 0], torch.tensor([0.0, 1.0])) and got["last_center"].shape[0] == Bl
    assert got["shared_table"] is ep["shared_table"] and got["note"] == "not a tensor"
    assert got["center_label"] is labels["center_label"] and got["scale"] is labels["scale"]
    assert not any(k.startswith("unlabeled.") for k in got) and "consistency_weight" not in got and "point_clouds" not in got
    # 2. the remaining scenes with the unlabelled batch's keys, unprefixed
    got, cfg, run_cfg, cd = calls["guide"]
    assert cfg is dataset and run_cfg is obj.config and cd is extra
    assert torch.equal(got["last_quad_center"][:, 0, 0], torch.tensor([2.0, 3.0, 4.0]))
    assert got["center_label"] is labels["unlabeled.center_label"] and got["point_clouds"] is labels["unlabeled.point_clouds"]
    assert got["shared_table"] is ep["shared_table"]
    # 3. the whole batch, with the augmentation of both batches concatenated in batch order, and the teacher's outputs
    got, got_teacher, cfg = calls["consistency"]
    assert got_teacher is teacher and cfg is dataset and got["last_quad_center"].shape[0] == Bl + Bu
    for i, key in enumerate(("flip_x_axis", "flip_y_axis", "rot_mat", "scale")):
        assert torch.equal(got[key][:, 0], torch.tensor([float(i)] * Bl + [100.0 + i] * Bu)), key
        assert got[key] is ep[key]                                   # written into the caller's end_points, as train.py:527 does
    # 4. the whole batch's predictions and the unlabelled batch
    got, unl, cfg = calls["arkit"]
    assert cfg is dataset and got["last_quad_center"].shape[0] == Bl + Bu
    assert set(unl) == {"center_label", "point_clouds", "flip_x_axis", "flip_y_axis", "rot_mat", "scale"}
    assert unl["center_label"] is labels["unlabeled.center_label"]
    want = SUP + CONS * 0.3 + (3.0 * METRICS[0] + 5.0 * METRICS[1] + 7.0 * METRICS[2] + 11.0 * METRICS[3]) + ARK * 0.75
    assert float(total) == pytest.approx(want, rel=1e-6)


@pytest.mark.parametrize("pc_loss, gamma_mixture, ema, arkit", list(itertools.product((False, True), repeat=4)))
def test_every_combination_of_the_switches(stubbed, pc_loss, gamma_mixture, ema, arkit):
    semi_objective, calls = stubbed
    ep, labels = batch()
    obj = semi_objective.SemiSupervisedObjective(None, config(pc_loss=pc_loss, gamma_mixture=gamma_mixture, ema=ema, arkit=arkit))
    total = obj(ep, labels, {} if ema else None)
    assert set(calls) == {"get_loss"} | ({"guide"} if gamma_mixture else set()) | ({"consistency"} if ema else set()) | \
        ({"arkit"} if arkit else set())
    assert calls["get_loss"][2] is pc_loss
    filt = 3.0 * METRICS[0] + 5.0 * METRICS[1] + 7.0 * METRICS[2] + 11.0 * METRICS[3]
    parts = {"loss": SUP, "consistency_loss": CONS * 0.3 if ema else 0.0, "gamma_mixture_filter_loss": filt if gamma_mixture else 0.0,
             "arkit_pc_loss": ARK * 0.75 if arkit else 0.0}
    assert float(total) == pytest.approx(sum(parts.values()), rel=1e-6)
    stats = obj.stats
    assert set(stats) == {"loss", "vote_loss", "box_loss", "physical_constraints_loss", "collisions", "metric_normal",
                          "metric_vertical", "metric_size", "metric_score", "gamma_mixture_filter_loss", "consistency_loss",
                          "arkit_pc_loss", "arkit_collisions", "total_loss"}
    for k, v in stats.items():
        assert torch.is_tensor(v) and v.dim() == 0 and v.dtype == torch.float32 and not v.requires_grad, k
    for k, want in parts.items():
        assert float(stats[k]) == pytest.approx(want, rel=1e-6), k
    assert float(stats["total_loss"]) == float(total) and float(stats["vote_loss"]) == 1.0
    assert float(stats["arkit_collisions"]) == (9.0 if arkit else 0.0)
    assert [float(stats[k]) for k in semi_objective.METRICS] == (list(METRICS) if gamma_mixture else [0.0] * 4)
    if not ema:                                                      # nothing was written into the caller's end_points
        assert "scale" not in ep


def test_a_batch_that_is_not_labelled_plus_unlabelled_is_refused(stubbed):
    semi_objective, calls = stubbed
    obj = semi_objective.SemiSupervisedObjective(None, config())
    ep, labels = batch(Bt=Bl + Bu + 1)
    with pytest.raises(ValueError, match="2 labelled \\+ 3 unlabelled"):
        obj(ep, labels, {})
    assert not calls
    ep, labels = batch()
    with pytest.raises(ValueError, match="teacher"):
        obj(ep, labels, None)                                        # config.ema without the teacher's outputs
    with pytest.raises(ValueError, match="both a label and an output"):
        obj(dict(ep, center_label=labels["center_label"]), labels, {})
    # without unlabelled tensors the batch is the labelled scenes alone
    obj = semi_objective.SemiSupervisedObjective(None, config(gamma_mixture=False, ema=False, arkit=False))
    ep, labels = batch(Bt=Bl)
    assert float(obj(ep, {k: v for k, v in labels.items() if not k.startswith("unlabeled.")})) == SUP
