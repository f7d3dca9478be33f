"""Dynamic fp16 loss scaling (optim.FusedAdamW(loss_scaler=...), CapturedStep(loss_scale="dynamic"); include/omnipq_optim.h:
omnipq_adamw_scaled_finalize) without a GPU: the float64 restatement the GPU tests use is held to torch itself, the libraries
report the entry point and the struct, every host-argument error comes back before a launch, and what the Python side accepts,
refuses and round-trips.

The bound of test 1b.  Per APPLIED step a parameter goes through two f32 roundings (p * (1 - lr wd), then the fused
multiply-add), each at most half an ulp, and ulp(x) <= 2^-23 |x|: together 2^-23 max|p|.  The update term lr * m^ / (sqrt(v^) +
eps) has |m^ / sqrt(v^)| < 4 over these few steps and carries the relative error of its chain of f32 roundings and of torch's
f32 norm over 2.6 M elements inside the clip coefficient, 2^-20 at the very most: lr * 4 * 2^-20.  So
    |p_torch_f32 - p_f64| <= applied steps * (2^-23 * max|p| + lr * 2^-18)
-- from the formats and the step count, not from a measurement.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import capi
import loss_scale_restatement as R
from test_fused_adamw_host import _Small, _groups
from test_gpu_fused_adamw import BETAS, EPS, GROUP, LRS, MAX_NORM, ULP, WD, groups_of, start_values

SIGNATURE = ("i", "ippii" + "p" * 9)
EINVAL = 10001


def _f32_bits(x):
    return np.float32(x).tobytes()


@pytest.mark.parametrize("init,schedule", [(R.INIT, R.SCHEDULE), (R.TOP, R.TOP_SCHEDULE)])
def test_restated_recurrence_is_torchs_amp_update_scale(init, schedule):
    """1a: scale and tracker after every step, bit for bit, against torch._amp_update_scale_ on CPU tensors"""
    scale, tracker = torch.full((1,), init, dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    s, t = float(np.float32(init)), 0
    seen = []
    for kind in schedule:
        found = torch.full((1,), 0.0 if kind == "finite" else 1.0)
        torch._amp_update_scale_(scale, tracker, found, R.GROWTH, R.BACKOFF, R.INTERVAL)
        s, t = R.update_scale(s, t, kind == "finite")
        assert _f32_bits(s) == scale.numpy().tobytes() and t == int(tracker), (kind, s, float(scale), t, int(tracker))
        seen.append((s / init, t))
    if init == R.INIT:       # every branch was walked: grown, backed off twice, tracker restarted, grown again
        assert seen == [(1, 1), (1, 2), (2, 0), (1, 0), (1, 1), (0.5, 0), (0.5, 1), (0.5, 2), (1, 0)]
    else:                    # 2^128 is not an f32: growth refused, the tracker reset all the same
        assert seen == [(1, 1), (1, 2), (1, 0)]
    # factors that are no powers of two round like torch's kernel does (f32 * f64 in f64, then once to f32)
    scale, tracker = torch.full((1,), 1000.0), torch.zeros(1, dtype=torch.int32)
    s, t = 1000.0, 0
    for found in (0, 0, 1, 0, 1, 1, 0, 0, 0, 0):
        torch._amp_update_scale_(scale, tracker, torch.full((1,), float(found)), 1.7, 0.3, 2)
        s, t = R.update_scale(s, t, not found, 1.7, 0.3, 2)
        assert _f32_bits(s) == scale.numpy().tobytes() and t == int(tracker)


@pytest.mark.parametrize("init,schedule", [(R.INIT, R.SCHEDULE), (R.TOP, R.TOP_SCHEDULE)])
def test_restatement_against_grad_scaler_clip_and_adamw_on_the_cpu(init, schedule):
    """1b: the whole recurrence against torch.amp.GradScaler("cpu") + clip_grad_norm_ + torch.optim.AdamW in f32"""
    vals, _ = start_values()
    truth = R.ScaledTruth(vals, init_scale=init)
    tparams = [torch.nn.Parameter(v.clone()) for v in vals]
    topt = torch.optim.AdamW(groups_of(tparams), lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    scaler = torch.amp.GradScaler("cpu", init_scale=init, growth_factor=R.GROWTH, backoff_factor=R.BACKOFF,
                                  growth_interval=R.INTERVAL)
    scaler.scale(torch.zeros(1))                                    # GradScaler creates its two tensors lazily
    applied = 0
    for kind, grads in zip(schedule, R.unscaled_grads(schedule)):
        assert scaler.get_scale() == truth.scale
        sg = R.scaled(grads, truth.scale, kind)
        for p, g in zip(tparams, sg):
            p.grad = None if g is None else g.clone()
        scaler.unscale_(topt)
        torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM, foreach=False)
        scaler.step(topt)
        scaler.update()
        norm, ok = truth.step(sg)
        assert ok == (kind == "finite") and math.isfinite(norm) == ok
        applied += ok
        assert _f32_bits(scaler.get_scale()) == _f32_bits(truth.scale), (kind, scaler.get_scale(), truth.scale)
        assert scaler._get_growth_tracker() == truth.tracker
    assert truth.t == applied == sum(k == "finite" for k in schedule) and truth.skipped == len(schedule) - applied
    assert float(topt.state[tparams[0]]["step"]) == applied        # torch skipped the same steps
    for i, (p, want) in enumerate(zip(tparams[:-1], truth.p[:-1])):
        err = float((p.detach().double() - want).abs().max())
        bound = applied * (ULP * float(want.abs().max()) + LRS[GROUP[i]] * 2.0 ** -18)
        print(f"tensor {i}: |torch f32 - restatement f64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (i, err, bound)
    assert torch.equal(tparams[-1].detach().double(), truth.p[-1])


def _declared_loss_scaler():
    """[(field, letter)] of `struct omnipq_loss_scaler` as include/omnipq_optim.h states it: this test's own reading"""
    import os
    import re
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(capi.INCLUDE, "omnipq_optim.h")).read(), flags=re.S)
    body = re.search(r"\bstruct\s+omnipq_loss_scaler\s*\{([^{}]*)\}\s*;", text).group(1)
    letters = {"float": "f", "int": "i"}
    return [(stmt.split()[1], letters[stmt.split()[0]]) for stmt in body.split(";") if stmt.strip()]


def test_entry_point_and_struct_are_declared_exported_and_reported(built_lib):
    """2a: the signature through the libraries' signature text; the struct's layout through omnipq_loss_scaler_record(), one
    line in the format of omnipq_abi_records() (whose own list of structs an existing test pins), against the header"""
    assert capi.declared_signatures()["omnipq_adamw_scaled_finalize"] == SIGNATURE
    assert capi.declared_signatures()["omnipq_loss_scaler_record"] == ("s", "")
    layout = _declared_loss_scaler()
    assert layout == [("scale", "f"), ("growth_tracker", "i")]
    want = "struct omnipq_loss_scaler " + " ".join(f"{f}:{t}" for f, t in layout)
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "omnipq_adamw_scaled_finalize")
        got = capi.reported_signatures(lib)
        assert got["omnipq_adamw_scaled_finalize"] == SIGNATURE and got["omnipq_loss_scaler_record"] == ("s", ""), path
        lib.omnipq_loss_scaler_record.restype = ctypes.c_char_p
        assert lib.omnipq_loss_scaler_record().decode() == want, path
        assert lib.omnipq_abi_version() == 5                      # an addition only
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    rec = ext.loss_scaler_struct()                                # the binding's class, built from that text
    assert rec is ext.loss_scaler_struct() and issubclass(rec, ctypes.Structure)
    assert ctypes.sizeof(rec) == 8 and rec.scale.offset == 0 and rec.growth_tracker.offset == 4
    assert rec._fields_ == [("scale", ctypes.c_float), ("growth_tracker", ctypes.c_int)]


def test_malformed_calls_return_einval_without_a_gpu(built_lib):
    """2b: nchunks, partials, hyper, ngroups, accum_steps, counters, accum, ema_state, ema_coef, scaler_cfg, scaler_state,
    result, coef"""
    import pointnet2_utils
    fin = pointnet2_utils._load_ext()._lib0.omnipq_adamw_scaled_finalize
    p, null = ctypes.c_void_p(0x1000), None                      # "some non-null pointer": validation comes first

    def call(nchunks=4, partials=p, hyper=p, ngroups=2, accum_steps=1, counters=p, accum=null, ema_state=null, ema_coef=null,
             scaler_cfg=p, scaler_state=p, result=p, coef=p):
        return fin(nchunks, partials, hyper, ngroups, accum_steps, counters, accum, ema_state, ema_coef, scaler_cfg,
                   scaler_state, result, coef, None)

    for bad in (dict(scaler_cfg=null), dict(scaler_state=null),                     # no scaler
                dict(ema_state=p), dict(ema_coef=p),                                # one of the teacher's pair without the other
                dict(accum_steps=3), dict(accum_steps=2, ema_state=p, ema_coef=p),  # micro-batches without their counter
                dict(accum_steps=0), dict(accum_steps=0, accum=p), dict(accum_steps=-1, accum=p),
                dict(nchunks=-1), dict(partials=null), dict(hyper=null), dict(ngroups=0), dict(counters=null),
                dict(result=null), dict(coef=null)):                                # what the other finalise calls refuse
        assert call(**bad) == EINVAL, bad


def test_loss_scaler_validates_like_torch():
    """3a"""
    import optim
    s = optim.LossScaler()
    t = torch.amp.GradScaler("cpu")
    assert (s.init_scale, s.growth_factor, s.backoff_factor, s.growth_interval) == \
        (t.get_scale(), t.get_growth_factor(), t.get_backoff_factor(), t.get_growth_interval()) == (65536.0, 2.0, 0.5, 2000)
    for bad in (dict(init_scale=0.0), dict(init_scale=-1.0), dict(init_scale=float("inf")), dict(init_scale=float("nan")),
                dict(init_scale=1e39), dict(init_scale="65536"),
                dict(growth_factor=1.0), dict(growth_factor=0.5), dict(growth_factor=float("nan")),
                dict(backoff_factor=1.0), dict(backoff_factor=0.0), dict(backoff_factor=-0.5), dict(backoff_factor=2.0),
                dict(backoff_factor=float("nan")),
                dict(growth_interval=0), dict(growth_interval=-3), dict(growth_interval=2.0), dict(growth_interval=True)):
        with pytest.raises(ValueError, match="LossScaler"):
            optim.LossScaler(**bad)
    assert optim.LossScaler(2 ** 14, 1.5, 0.25, 1).growth_interval == 1


def test_optimizer_carries_the_scaler_and_round_trips_grad_scalers_state(built_lib):
    """3b: opt.loss_scale is a view of the device struct; scaler_state_dict() has GradScaler.state_dict()'s keys and types and
    each loads what the other wrote; snapshot / restore carry scale and tracker; state_dict() stays torch.optim.AdamW's"""
    import optim
    torch.manual_seed(0)
    net = _Small()
    plain = optim.FusedAdamW(_groups(net), lr=2e-3)
    assert plain.loss_scaler is None and plain.loss_scale is None and plain.scale_value is None and plain.growth_tracker is None
    assert tuple(plain.staging.shape) == (3, 8)
    with pytest.raises(RuntimeError, match="loss_scaler"):
        plain.scaler_state_dict()
    with pytest.raises(ValueError, match="LossScaler"):
        optim.FusedAdamW(_groups(net), lr=2e-3, loss_scaler=torch.amp.GradScaler("cpu"))
    cfg = optim.LossScaler(init_scale=2.0 ** 14, growth_interval=7)
    opt = optim.FusedAdamW(_groups(net), lr=2e-3, max_norm=0.1, grad_scale=0.5, loss_scaler=cfg)
    assert opt.loss_scale.dtype == torch.float32 and opt.loss_scale.dim() == 0
    assert opt.loss_scale.untyped_storage().data_ptr() == opt.scaler_state.untyped_storage().data_ptr()        # a view
    assert opt.scaler_state.numel() == 8 and opt.scale_value == 2.0 ** 14 and opt.growth_tracker == 0
    assert opt.scaler_state.view(torch.float32)[0].item() == 2.0 ** 14 and opt.scaler_state.view(torch.int32)[1].item() == 0
    # the factors are one more staged row, behind the rows the other launches index
    assert tuple(opt.staging.shape) == (4, 8)
    assert opt.staging[2, :3].tolist() == [0.1, 0.5, 0.0] and opt.staging[3].tolist() == [2.0, 0.5, 7.0, 0, 0, 0, 0, 0]
    assert opt.sync_hyperparameters() is False
    opt.loss_scaler.growth_interval = 9
    assert opt.sync_hyperparameters() is True and opt.staging[3, 2].item() == 9.0
    assert cfg.growth_interval == 7                                # the optimiser changed its own copy
    opt.loss_scaler.growth_interval = 0
    with pytest.raises(ValueError, match="growth_interval"):
        opt.sync_hyperparameters()
    opt.loss_scaler.growth_interval = 9
    # -> GradScaler
    ours = opt.scaler_state_dict()
    theirs = torch.amp.GradScaler("cpu").state_dict()
    assert list(ours) == list(theirs) == ["scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"]
    assert [type(v) for v in ours.values()] == [type(v) for v in theirs.values()] == [float, float, float, int, int]
    assert ours == {"scale": 2.0 ** 14, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 9, "_growth_tracker": 0}
    gs = torch.amp.GradScaler("cpu")
    gs.load_state_dict(ours)
    assert gs.state_dict() == ours
    # <- GradScaler, after it has moved
    gs = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=5)
    gs.scale(torch.zeros(1))
    torch._amp_update_scale_(gs._scale, gs._growth_tracker, torch.zeros(1), 3.0, 0.25, 5)
    theirs = gs.state_dict()
    assert theirs["_growth_tracker"] == 1
    opt.load_scaler_state_dict(theirs)
    assert opt.scaler_state_dict() == theirs and opt.scale_value == 1024.0 and opt.growth_tracker == 1
    assert opt.staging[3, :3].tolist() == [3.0, 0.25, 5.0]
    for spoil in (dict(scale=0.0), dict(growth_factor=1.0), dict(backoff_factor=1.5), dict(growth_interval=0),
                  dict(_growth_tracker=-1), dict(_growth_tracker=1.5)):
        with pytest.raises(ValueError):
            opt.load_scaler_state_dict(dict(theirs, **spoil))
    with pytest.raises(RuntimeError, match="empty"):
        opt.load_scaler_state_dict(torch.amp.GradScaler("cpu", enabled=False).state_dict())
    assert opt.scaler_state_dict() == theirs                       # a refused dict changed nothing
    # snapshot / restore
    saved = opt.snapshot()
    with torch.no_grad():
        opt.loss_scale.mul_(0.5)
        opt._tracker.fill_(0)
    assert opt.scale_value == 512.0
    opt.restore(saved)
    assert opt.scale_value == 1024.0 and opt.growth_tracker == 1
    # state_dict() knows nothing of the scaler
    ref = torch.optim.AdamW(_groups(net), lr=2e-3).state_dict()
    got = opt.state_dict()
    assert set(got) == set(ref) and [set(g) for g in got["param_groups"]] == [set(g) for g in ref["param_groups"]]
    net(torch.randn(4, 5)).sum().backward()
    with pytest.raises(RuntimeError, match="CPU not supported"):
        opt.step()


def test_captured_step_takes_dynamic_only_with_a_scaler_carrying_optimizer(built_lib):
    """3c: each mismatch raises before anything touches a device"""
    import optim
    import train_step
    torch.manual_seed(0)
    net = _Small()

    def build(**kw):
        return train_step.CapturedStep(net, lambda ep, lab: ep, torch.zeros(1, 4, 3), graph=False, prefetch=None, **kw)

    def fused(**kw):
        return optim.FusedAdamW(_groups(net), lr=2e-3, **kw)

    for kw in (dict(loss_scale="dynamic"),                                               # no in-graph optimizer
               dict(loss_scale="dynamic", optimizer=fused()),                            # ... one without a scaler
               dict(loss_scale="Dynamic", optimizer=fused(loss_scaler=optim.LossScaler())),
               dict(loss_scale=2.0 ** 14, optimizer=fused(loss_scaler=optim.LossScaler())),      # a static scale on top
               dict(loss_scale=0.5, optimizer=fused(loss_scaler=optim.LossScaler()))):
        with pytest.raises(ValueError, match="loss_scale="):
            build(**kw)
    opt = fused(loss_scaler=optim.LossScaler(init_scale=2.0 ** 10), grad_scale=0.25)
    st = build(loss_scale="dynamic", optimizer=opt)
    assert st.dynamic_scale is True and st.scale == 1.0 and opt.grad_scale == 0.25 and opt.scale_value == 2.0 ** 10
    # _backward multiplies by the device tensor itself
    seen = []
    st.defer = False
    x = torch.ones((), requires_grad=True)
    loss = x * 3.0
    loss.register_hook(seen.append)
    st._backward(loss)
    assert float(seen[-1]) == 2.0 ** 10 and float(x.grad) == 3.0 * 2.0 ** 10
    # a scaler-carrying optimizer with the default loss_scale=1 is left to a criterion that scales by itself
    st1 = build(optimizer=fused(loss_scaler=optim.LossScaler()))
    assert st1.dynamic_scale is False and st1.scale == 1.0
    # the static route is what it was
    o2 = fused()
    st2 = build(loss_scale=2.0 ** 14, optimizer=o2)
    assert st2.dynamic_scale is False and st2.scale == 2.0 ** 14 and o2.grad_scale == 2.0 ** -14
