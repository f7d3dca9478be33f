"""omni-pq_amd/optim.py + include/omnipq_optim.h without a GPU: the entry points exist and validate their arguments on the
host, FusedAdamW's state_dict is torch.optim.AdamW's in both directions, what it refuses, and the rows an LR scheduler makes
`sync_hyperparameters()` stage."""
import ctypes

import numpy as np
import pytest
import torch

import capi

ENTRY_POINTS = {"omnipq_adamw_check_table": ("i", "ipipii"), "omnipq_adamw_grad_sqnorm": ("i", "iippipipp"),
                "omnipq_adamw_finalize": ("i", "ippipppp"), "omnipq_adamw_update": ("i", "iippippp")}
EINVAL = 10001


def test_entry_points_are_declared_exported_and_reported(built_lib):
    declared = capi.declared_signatures()
    for name, sig in ENTRY_POINTS.items():
        assert declared[name] == sig, name
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        for name, sig in ENTRY_POINTS.items():
            assert hasattr(lib, name) and got[name] == sig, (path, name)
        assert lib.omnipq_abi_version() == 5                      # additions only


def _records(n, group=0, numel=5000):
    import optim
    rec = np.zeros(n, dtype=optim.RECORD)
    assert rec.itemsize == 48
    for i in range(n):
        rec[i] = (0x1000, 0x2000, 0x3000, 0x4000, numel, group, 0)      # never dereferenced
    return rec


def test_malformed_calls_return_einval_without_a_gpu(built_lib):
    import pointnet2_utils
    lib = pointnet2_utils._load_ext()._lib0
    p, null = ctypes.c_void_p(0x1000), None                      # "some non-null pointer": validation comes first
    # launches: null tables, negative counts, no hyper-parameter rows, chunk sizes that are not multiples of 1024
    assert lib.omnipq_adamw_grad_sqnorm(2, 4, null, p, 4096, p, 2, p, None) == EINVAL
    assert lib.omnipq_adamw_grad_sqnorm(2, 4, p, null, 4096, p, 2, p, None) == EINVAL
    assert lib.omnipq_adamw_grad_sqnorm(2, 4, p, p, 4096, null, 2, p, None) == EINVAL
    assert lib.omnipq_adamw_grad_sqnorm(2, 4, p, p, 4096, p, 2, null, None) == EINVAL
    assert lib.omnipq_adamw_grad_sqnorm(-1, 4, p, p, 4096, p, 2, p, None) == EINVAL
    assert lib.omnipq_adamw_grad_sqnorm(2, -4, p, p, 4096, p, 2, p, None) == EINVAL
    assert lib.omnipq_adamw_grad_sqnorm(2, 4, p, p, 4096, p, 0, p, None) == EINVAL
    assert lib.omnipq_adamw_grad_sqnorm(2, 4, p, p, 1000, p, 2, p, None) == EINVAL
    assert lib.omnipq_adamw_grad_sqnorm(0, 0, null, null, 4096, p, 2, null, None) == 0          # nothing to do
    assert lib.omnipq_adamw_finalize(-1, p, p, 2, p, p, p, None) == EINVAL
    assert lib.omnipq_adamw_finalize(4, null, p, 2, p, p, p, None) == EINVAL
    assert lib.omnipq_adamw_finalize(4, p, null, 2, p, p, p, None) == EINVAL
    assert lib.omnipq_adamw_finalize(4, p, p, 0, p, p, p, None) == EINVAL
    assert lib.omnipq_adamw_finalize(4, p, p, 2, null, p, p, None) == EINVAL
    assert lib.omnipq_adamw_finalize(4, p, p, 2, p, null, p, None) == EINVAL
    assert lib.omnipq_adamw_finalize(4, p, p, 2, p, p, null, None) == EINVAL
    assert lib.omnipq_adamw_update(2, 4, null, p, 4096, p, p, None) == EINVAL
    assert lib.omnipq_adamw_update(2, 4, p, null, 4096, p, p, None) == EINVAL
    assert lib.omnipq_adamw_update(2, 4, p, p, 4096, null, p, None) == EINVAL
    assert lib.omnipq_adamw_update(2, 4, p, p, 4096, p, null, None) == EINVAL
    assert lib.omnipq_adamw_update(-2, 4, p, p, 4096, p, p, None) == EINVAL
    assert lib.omnipq_adamw_update(2, -4, p, p, 4096, p, p, None) == EINVAL
    assert lib.omnipq_adamw_update(2, 4, p, p, 4097, p, p, None) == EINVAL
    assert lib.omnipq_adamw_update(0, 0, null, null, 4096, p, p, None) == 0

    # the host copy of a table: groups outside the hyper-parameter rows, null tensors, chunks outside their record
    def check(rec, chunks, ngroups=2, chunk=4096):
        chunks = np.asarray(chunks, dtype=np.int32).reshape(-1, 2)
        return lib.omnipq_adamw_check_table(len(rec), rec.ctypes.data_as(ctypes.c_void_p), len(chunks),
                                            chunks.ctypes.data_as(ctypes.c_void_p), ngroups, chunk)

    good = [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert check(_records(2), good) == 0
    assert check(_records(2, group=1), good) == 0
    assert check(_records(2, group=2), good) == EINVAL
    assert check(_records(2, group=-1), good) == EINVAL
    assert check(_records(2, numel=-1), []) == EINVAL
    assert check(_records(2), good + [(2, 0)]) == EINVAL          # no such record
    assert check(_records(2), good + [(1, 2)]) == EINVAL          # 2 * 4096 >= 5000: past the record's last element
    assert check(_records(2), good + [(1, -1)]) == EINVAL
    assert check(_records(2), good, ngroups=0) == EINVAL
    assert check(_records(2), good, chunk=100) == EINVAL
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        rec = _records(2)
        rec[field][1] = 0
        assert check(rec, good) == EINVAL, field
        rec[field][1] = 0x1002                                     # not 4-byte aligned
        assert check(rec, good) == EINVAL, field
    assert lib.omnipq_adamw_check_table(2, None, 0, None, 2, 4096) == EINVAL
    assert lib.omnipq_adamw_check_table(-1, None, 0, None, 2, 4096) == EINVAL


class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = torch.nn.Linear(5, 7)
        self.decoder = torch.nn.Sequential(torch.nn.Linear(7, 3), torch.nn.LayerNorm(3))

    def forward(self, x):
        return self.decoder(self.backbone(x))


def _groups(net):
    """the reference's two groups (train.py:365-371)"""
    return [{"params": [p for n, p in net.named_parameters() if "decoder" not in n and p.requires_grad]},
            {"params": [p for n, p in net.named_parameters() if "decoder" in n and p.requires_grad], "lr": 1e-4}]


def _two_torch_steps(net):
    opt = torch.optim.AdamW(_groups(net), lr=2e-3, weight_decay=5e-4)
    torch.manual_seed(1)
    for _ in range(2):
        opt.zero_grad()
        net(torch.randn(4, 5)).square().sum().backward()
        opt.step()
    return opt


def _same_structure(a, b):
    assert set(a) == set(b) == {"state", "param_groups"}
    assert len(a["param_groups"]) == len(b["param_groups"])
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert set(ga) == set(gb)
        for k in ga:
            assert ga[k] == gb[k], k
    assert set(a["state"]) == set(b["state"])
    for idx in a["state"]:
        assert set(a["state"][idx]) == set(b["state"][idx]) == {"step", "exp_avg", "exp_avg_sq"}
        for k, v in a["state"][idx].items():
            w = b["state"][idx][k]
            assert torch.is_tensor(v) and torch.is_tensor(w) and v.dtype == w.dtype and v.shape == w.shape, (idx, k)
            assert torch.equal(v, w), (idx, k)


def test_state_dict_round_trip_with_torch_adamw(built_lib):
    import optim
    torch.manual_seed(0)
    net = _Small()
    want = _two_torch_steps(net).state_dict()
    assert len(want["state"]) == 6 and float(want["state"][0]["step"]) == 2.0
    fused = optim.FusedAdamW(_groups(net), lr=1.0, weight_decay=0.0)             # own values: the loaded groups replace them
    fused.load_state_dict(want)
    assert fused.t == 2 and fused.skipped == 0
    got = fused.state_dict()
    _same_structure(got, want)
    # the moments ARE the flat buffers: state[p] holds views into them
    for g in fused.param_groups:
        assert g["lr"] in (2e-3, 1e-4) and g["weight_decay"] == 5e-4
        for p in g["params"]:
            st = fused.state[p]
            assert st["exp_avg"].untyped_storage().data_ptr() == fused.exp_avg.untyped_storage().data_ptr()
            assert st["exp_avg_sq"].untyped_storage().data_ptr() == fused.exp_avg_sq.untyped_storage().data_ptr()
            assert st["exp_avg"].data_ptr() % 16 == p.data_ptr() % 16           # moments share the parameter's 16-byte phase
    # ... and a fresh torch.optim.AdamW loads that state in turn
    back = torch.optim.AdamW(_groups(net), lr=1.0)
    back.load_state_dict(got)
    _same_structure(back.state_dict(), want)
    # a fresh FusedAdamW has torch's fresh state_dict: no per-parameter state yet
    fresh = optim.FusedAdamW(_groups(net), lr=2e-3, weight_decay=5e-4).state_dict()
    ref = torch.optim.AdamW(_groups(net), lr=2e-3, weight_decay=5e-4).state_dict()
    assert fresh["state"] == {} == ref["state"]
    assert [set(g) for g in fresh["param_groups"]] == [set(g) for g in ref["param_groups"]]
    for ga, gb in zip(fresh["param_groups"], ref["param_groups"]):
        assert ga == gb


def test_checkpoint_file_of_either_optimizer_loads_into_the_other(built_lib, tmp_path):
    import argparse
    import checkpoint
    import optim
    torch.manual_seed(0)
    net = _Small()
    topt = _two_torch_steps(net)
    sched = torch.optim.lr_scheduler.StepLR(topt, 10)
    args = argparse.Namespace(log_dir=str(tmp_path), save_freq=1, checkpoint_path=None)
    args.checkpoint_path = checkpoint.save_checkpoint(args, 3, net, topt, sched, save_cur=True)
    fused = optim.FusedAdamW(_groups(net), lr=2e-3, weight_decay=5e-4)
    fsched = torch.optim.lr_scheduler.StepLR(fused, 10)
    assert checkpoint.load_checkpoint(args, net, fused, fsched) == 3
    _same_structure(fused.state_dict(), topt.state_dict())
    args.checkpoint_path = checkpoint.save_checkpoint(args, 4, net, fused, fsched, save_cur=True)
    again = torch.optim.AdamW(_groups(net), lr=2e-3, weight_decay=5e-4)
    checkpoint.load_checkpoint(args, net, again, torch.optim.lr_scheduler.StepLR(again, 10))
    _same_structure(again.state_dict(), topt.state_dict())


def test_refusals(built_lib):
    import optim
    torch.manual_seed(0)
    net = _Small()
    state = _two_torch_steps(net).state_dict()
    state["state"][3]["step"] = torch.tensor(5.0)
    fused = optim.FusedAdamW(_groups(net), lr=2e-3)
    with pytest.raises(ValueError, match="step"):
        fused.load_state_dict(state)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        optim.FusedAdamW(_groups(net), lr=2e-3, amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        optim.FusedAdamW(_groups(net), lr=2e-3, maximize=True)
    net(torch.randn(4, 5)).sum().backward()
    with pytest.raises(RuntimeError, match="CPU not supported"):
        fused.step()
    import train_step
    with pytest.raises(TypeError, match="FusedAdamW"):
        train_step.CapturedStep(net, lambda ep, lab: ep, torch.zeros(1, 4, 3), graph=False, prefetch=None,
                                optimizer=torch.optim.AdamW(net.parameters()))
    with pytest.raises(ValueError, match="accumulation"):
        train_step.CapturedStep(net, lambda ep, lab: ep, torch.zeros(1, 4, 3), graph=False, prefetch=None, optimizer=fused,
                                step_freq=2)
    st = train_step.CapturedStep(net, lambda ep, lab: ep, torch.zeros(1, 4, 3), graph=False, prefetch=None, optimizer=fused,
                                 loss_scale=2.0 ** 14)
    assert fused.grad_scale == 2.0 ** -14 and st.optimizer is fused


def test_scheduler_changes_the_staged_rows(built_lib):
    import optim
    torch.manual_seed(0)
    net = _Small()
    fused = optim.FusedAdamW(_groups(net), lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4, max_norm=0.1,
                             grad_scale=0.5)
    rows = fused.staging
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (3, 8)
    assert rows[0, :5].tolist() == [2e-3, 0.9, 0.999, 1e-8, 5e-4] and rows[1, :5].tolist() == [1e-4, 0.9, 0.999, 1e-8, 5e-4]
    assert rows[2, :2].tolist() == [0.1, 0.5]
    assert fused.sync_hyperparameters() is False                   # nothing changed: nothing is sent
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(fused, T_max=10)
    fused._opt_called = True
    sched.step()
    lr0, lr1 = (g["lr"] for g in fused.param_groups)
    assert lr0 < 2e-3 and lr1 < 1e-4
    assert fused.sync_hyperparameters() is True
    rows = fused.staging
    assert rows[0, 0].item() == lr0 and rows[1, 0].item() == lr1
    assert rows[0, 1:5].tolist() == [0.9, 0.999, 1e-8, 5e-4] and rows[2, :2].tolist() == [0.1, 0.5]
    fused.max_norm = 0.2
    assert fused.sync_hyperparameters() is True and fused.staging[2, 0].item() == 0.2
