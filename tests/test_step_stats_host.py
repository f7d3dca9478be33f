"""Windowed step statistics (step_stats.StepStats; include/omnipq_optim.h: omnipq_stats_accumulate) without a GPU: which keys
train.py:581's rule selects, how a window's sums become means, and the entry point's argument checks."""
import ctypes

import pytest
import torch

import capi

EINVAL = 10001


def test_select_applies_the_references_rule():
    """a dict shaped like get_loss's end_points plus objective.stats: 0-dim tensors, Python floats, tensors that are no
    scalars, keys that match none of 'loss' / 'acc' / 'ratio'"""
    import step_stats
    ep = {
        "loss": torch.tensor(1.5), "0head_box_loss": torch.tensor(0.25), "last_sem_cls_loss": torch.tensor(2.0),
        "proposal_obj_acc": torch.tensor(0.5, dtype=torch.float64), "pos_ratio": torch.tensor(0.125),
        "quad_loss": 0.0, "consistency_loss": 0.0,                          # the reference's placeholders
        "center": torch.zeros(2, 8, 3), "objectness_scores": torch.zeros(2, 8, 2),      # no statistics: not selected by name
        "objectness_loss_mask": torch.zeros(2, 8),                           # selected by name, no scalar
        "acc_count": torch.tensor(3),                                        # selected by name, no floating point
        "acc_flag": True, "loss_weights": [1.0, 2.0], "loss_name": "huber",   # neither a float nor a tensor
        "sa1_inds": torch.zeros(4, dtype=torch.int32), "grad_norm": torch.tensor(9.0), 7: torch.tensor(1.0),
    }
    tensors, constants = step_stats.StepStats.select(ep)
    assert list(tensors) == ["loss", "0head_box_loss", "last_sem_cls_loss", "proposal_obj_acc", "pos_ratio"]
    assert all(tensors[k] is ep[k] for k in tensors)
    assert constants == {"quad_loss": 0.0, "consistency_loss": 0.0}
    # every key the reference's loop would have touched is accounted for, and no other
    touched = [k for k in ep if isinstance(k, str) and ("loss" in k or "acc" in k or "ratio" in k)]
    assert set(tensors) | set(constants) == set(touched) - {"objectness_loss_mask", "acc_count", "acc_flag", "loss_weights",
                                                            "loss_name"}
    assert step_stats.StepStats.select({}) == ({}, {})


def test_window_means_divide_like_the_reference():
    import step_stats
    w = step_stats.Window({"loss": 6.0, "acc": 1.5, "grad_norm": 0.75}, {"loss": 2.5, "acc": 0.5, "grad_norm": 0.75}, 3, 9,
                          last_mode=("grad_norm",))
    assert dict(w) == {"loss": 6.0, "acc": 1.5, "grad_norm": 0.75} and (w.steps, w.calls) == (3, 9)
    assert w.means() == {"loss": 2.0, "acc": 0.5, "grad_norm": 0.75}                 # by the steps accumulated
    assert w.means(10) == {"loss": 6.0 / 10, "acc": 1.5 / 10, "grad_norm": 0.75}     # by print_freq, as train.py:591 divides
    assert w.last["loss"] == 2.5
    with pytest.raises(ZeroDivisionError):
        step_stats.Window({"loss": 0.0}, {"loss": 0.0}, 0, 2).means()


def test_python_side_refuses_what_it_cannot_launch():
    import step_stats
    s = step_stats.StepStats()
    with pytest.raises(RuntimeError, match="nothing was accumulated"):
        s.read()
    with pytest.raises(ValueError, match="between 1 and 4096"):
        s.accumulate({"center": torch.zeros(3)})
    with pytest.raises(ValueError, match="between 1 and 4096"):
        s.accumulate({f"loss{i}": torch.tensor(0.0) for i in range(4097)})
    with pytest.raises(RuntimeError, match="CPU not supported"):
        s.accumulate({"loss": torch.tensor(1.0)})


def test_malformed_calls_return_einval_without_a_gpu(built_lib):
    """n = 0, n = 4097 and null tables come back before anything is launched; the signature is the header's"""
    import pointnet2_utils
    lib = pointnet2_utils._load_ext()._lib0
    assert capi.declared_signatures()["omnipq_stats_accumulate"] == ("i", "ipppppp")
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        assert capi.reported_signatures(ctypes.CDLL(path))["omnipq_stats_accumulate"] == ("i", "ipppppp")
    p, null = ctypes.c_void_p(0x1000), None

    def call(n=3, entries=p, sums=p, last=p, window=p, accum=null):
        return lib.omnipq_stats_accumulate(n, entries, sums, last, window, accum, None)

    for bad in (dict(n=0), dict(n=-1), dict(n=4097), dict(n=1 << 30), dict(entries=null), dict(sums=null), dict(last=null),
                dict(window=null), dict(n=4097, accum=p)):
        assert call(**bad) == EINVAL, bad
