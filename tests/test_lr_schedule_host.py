"""The learning-rate schedule on the device (optim.LRSchedule, FusedAdamW(lr_schedule=...); include/omnipq_optim.h: struct
omnipq_lr_schedule, omnipq_lr_schedule_eval, omnipq_adamw_sched_finalize) without a GPU: the float64 restatement the GPU tests
use (tests/lr_schedule_restatement.py) is held to the reference's own schedulers through tests/golden/lr_schedule.npz and to
torch's closed forms, the libraries report the struct and the entry points, every host-argument error comes back before a
launch, and what the Python object accepts, refuses and round-trips.
"""
import ctypes
import json
import os
import re
import warnings
from collections import Counter

import numpy as np
import pytest
import torch

import capi
import lr_schedule_restatement as R
from conftest import GOLDEN

EINVAL = 10001
FINALIZE = ("i", "ippii" + "p" * 13)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "lr_schedule.npz"))


def _bits(xs):
    return np.asarray(xs, dtype=np.float64).tobytes()


def _dict(golden, name, e):
    """the fixture's state_dict as the reference held it: MultiStepLR's milestones are a Counter of ints"""
    def back(d):
        d = dict(d)
        if "milestones" in d:
            d["milestones"] = Counter({int(k): v for k, v in d["milestones"]["__counter__"].items()})
        if "after_scheduler" in d:
            d["after_scheduler"] = back(d["after_scheduler"])
        return d
    return back(json.loads(str(golden[f"{name}/dict{e}"])))


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_is_the_references_schedule(golden, name):
    """1: with a warm-up bit for bit; without one within 4 x the drift of torch's recursive forms recorded in the fixture (the
    margin covers another libm, not another formula)"""
    want = golden[f"{name}/lrs"]
    s = R.case(name)
    got = np.asarray([s.lrs(e) for e in range(R.STEPS + 1)])
    assert want.shape == got.shape == (R.STEPS + 1, 2)
    if R.CASES[name][1] > 0:
        assert float(golden[f"{name}/maxrel"]) == 0.0
        assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:4]
    else:
        recorded = float(golden[f"{name}/maxrel"])
        rel = float(np.max(np.abs(got - want) / want))
        assert 0.0 < recorded < 1e-14
        assert rel <= 4 * recorded, f"{name}: max relative difference {rel:.3e}, bound {4 * recorded:.3e} = 4 x recorded {recorded:.3e}"


def _torch_closed_form(kind, s, steps):
    p = [torch.nn.Parameter(torch.zeros(1)) for _ in R.BASE_LRS]
    opt = torch.optim.SGD([{"params": [q], "lr": lr} for q, lr in zip(p, R.BASE_LRS)])
    if kind == "cosine":
        sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=s.t_max, eta_min=s.eta_min)
    else:
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(s.milestones), gamma=s.gamma)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in steps:
            sch.step(k)                      # an explicit epoch: torch takes _get_closed_form_lr
            out.append([g["lr"] for g in opt.param_groups])
    return out


@pytest.mark.parametrize("kind", ["cosine", "step"])
def test_restatement_is_torchs_closed_form(kind):
    """2: 200 steps against CosineAnnealingLR / MultiStepLR stepped with an explicit epoch, bit for bit -- the restatement and
    the product's host formulas (optim.LRSchedule.lr_at, what state_dict() reports without a GPU) alike"""
    import optim
    args = (kind, R.N_ITER, R.MAX_EPOCH, -1, R.MULTIPLIER, R.DECAY_EPOCHS, R.DECAY_RATE)
    s, mine = R.Schedule(*args), optim.LRSchedule(*args)
    steps = list(range(1, 201))
    want = _torch_closed_form(kind, s, steps)
    got = [s.lrs(k) for k in steps]
    assert _bits(got) == _bits(want)
    assert _bits([[mine.lr_at(k, b) for b in R.BASE_LRS] for k in steps]) == _bits(want)


def test_edge_cases_of_the_restatement():
    """3: e = W and W + 1, W = 1, T_max = 1, e > T_max, duplicate milestones, a milestone at k = 0, too many milestones"""
    import optim
    b0, b1 = R.BASE_LRS
    # e == W is the warm-up's last value -- not b for every b -- and e == W + 1 the after-scheduler's k = 1
    s = R.case("cosine_warm")
    w = s.warmup_iters
    assert w == 14 and s.lr(w, b0) == b0 and s.lr(w, b1) == 9.999999999999999e-05 != b1
    assert s.lr(w, b1) == b1 / 100 * ((100 - 1.) * w / w + 1.)
    assert _bits([s.lrs(w + 1)]) == _bits(_torch_closed_form("cosine", s, [1]))
    assert s.lr(0, b0) == b0 / 100
    # W = 1: one warm-up value behind the start, then k = e - 1
    s1 = R.Schedule("step", 1, 12, 1, 100, (1, 3), 0.1)
    assert s1.warmup_iters == 1 and s1.milestones == [0, 2]                 # a milestone at k = 0
    assert s1.lr(0, b0) == b0 / 100 and s1.lr(1, b0) == b0 / 100 * ((100 - 1.) * 1 / 1 + 1.)
    assert [s1.lr(e, b0) for e in (2, 3, 4)] == [b0 * 0.1 ** 1, b0 * 0.1 ** 2, b0 * 0.1 ** 2]
    assert _bits([s1.lrs(e) for e in (2, 3, 4, 9)]) == _bits(_torch_closed_form("step", s1, [1, 2, 3, 8]))
    # ... and without a warm-up the milestone at k = 0 counts from e = 0 on
    s0 = R.Schedule("step", 2, 5, -1, 100, (-1, 1), 0.5)
    assert s0.milestones == [0, 4] and s0.lr(0, b0) == b0 * 0.5 and s0.lr(4, b0) == b0 * 0.25
    # T_max = 1 and e > T_max: the cosine goes on, as torch's closed form does
    st = R.Schedule("cosine", 1, 0, -1)
    assert st.t_max == 1
    ks = [0, 1, 2, 3, 7]
    assert _bits([st.lrs(k) for k in ks][1:]) == _bits(_torch_closed_form("cosine", st, ks[1:]))
    assert st.lr(1, b0) == st.eta_min
    long = R.case("cosine_cold")
    ks = [long.t_max - 1, long.t_max, long.t_max + 1, 2 * long.t_max, 3 * long.t_max + 5]
    assert _bits([long.lrs(k) for k in ks]) == _bits(_torch_closed_form("cosine", long, ks))
    # duplicate milestones count once each
    sd = R.Schedule("step", 1, 20, -1, 100, (3, 3, 6), 0.1)
    assert sd.milestones == [4, 4, 7] and sd.lr(4, b0) == b0 * 0.1 ** 2 and sd.lr(7, b0) == b0 * 0.1 ** 3
    assert _bits([sd.lrs(k) for k in range(1, 10)]) == _bits(_torch_closed_form("step", sd, range(1, 10)))
    # the product's host formulas are the same text
    for sched, args in ((s, ("cosine", R.N_ITER, R.MAX_EPOCH, 2, 100)), (s1, ("step", 1, 12, 1, 100, (1, 3), 0.1)),
                        (sd, ("step", 1, 20, -1, 100, (3, 3, 6), 0.1)), (st, ("cosine", 1, 0, -1))):
        mine = optim.LRSchedule(*args)
        assert _bits([[mine.lr_at(e, b) for b in R.BASE_LRS] for e in range(40)]) == _bits([sched.lrs(e) for e in range(40)])
    # more milestones than the library's struct holds
    assert optim.LRSchedule.max_milestones() == R.MAX_MILESTONES == 8
    optim.LRSchedule("step", 1, 20, -1, 100, tuple(range(1, 9)), 0.1)
    with pytest.raises(ValueError, match="milestones"):
        optim.LRSchedule("step", 1, 20, -1, 100, tuple(range(1, 10)), 0.1)
    with pytest.raises(ValueError, match="milestones"):
        R.Schedule("step", 1, 20, -1, 100, tuple(range(1, 10)), 0.1)


def test_schedule_validates_its_host_copy_and_refuses_a_host_step():
    import optim
    import types
    with pytest.raises(NotImplementedError, match="scheduler poly not supported"):
        optim.LRSchedule("poly", 7, 12)
    with pytest.raises(NotImplementedError, match="scheduler poly not supported"):
        R.Schedule("poly", 7, 12)
    with pytest.raises(ValueError, match="T_max"):
        optim.LRSchedule("cosine", 7, 2, 2)
    with pytest.raises(ValueError, match="multiplier should be greater than 1."):
        optim.LRSchedule("cosine", 7, 12, 2, 1)
    s = optim.LRSchedule("cosine", 7, 12, 2)
    for name, bad in (("kind", "linear"), ("t_max", 0), ("warmup_iters", -1), ("multiplier", 1.0), ("milestones", [3, 1])):
        keep = getattr(s, name)
        setattr(s, name, bad)
        with pytest.raises(ValueError):
            s.validate()
        setattr(s, name, keep)
    s.validate()
    with pytest.raises(RuntimeError, match="stepped on the device"):
        s.step()
    with pytest.raises(RuntimeError, match="not attached"):
        s.state_dict()
    # from_args reads get_scheduler's names
    args = types.SimpleNamespace(lr_scheduler="step", max_epoch=12, warmup_epoch=2, warmup_multiplier=100, lr_decay_epochs=6,
                                 lr_decay_rate=0.1)
    a = optim.LRSchedule.from_args(args, 7)
    assert (a.kind, a.warmup_iters, a.multiplier, a.milestones, a.gamma, a.t_max) == ("step", 14, 100, [28], 0.1, 70)
    c = optim.LRSchedule.from_args(types.SimpleNamespace(lr_scheduler="cosine", max_epoch=12, warmup_epoch=-1), 7)
    assert (c.kind, c.warmup_iters, c.t_max, c.eta_min, c.milestones) == ("cosine", 0, 91, 1e-6, [])


def _attached(name):
    import optim
    kind, warm = R.CASES[name]
    params = [torch.nn.Parameter(torch.zeros(3)) for _ in R.BASE_LRS]
    s = optim.LRSchedule(kind, R.N_ITER, R.MAX_EPOCH, warm, R.MULTIPLIER, R.DECAY_EPOCHS, R.DECAY_RATE)
    opt = optim.FusedAdamW([{"params": [p], "lr": lr} for p, lr in zip(params, R.BASE_LRS)], lr_schedule=s)
    return s, opt


def _same_dict(got, want, exact, bound, where):
    assert set(got) == set(want), (where, set(got) ^ set(want))
    for k in want:
        if k == "after_scheduler":
            _same_dict(got[k], want[k], exact, bound, where + ".after_scheduler")
        elif k == "_last_lr" and not exact:
            rel = max(abs(a - b) / b for a, b in zip(got[k], want[k]))
            assert rel <= bound, f"{where}._last_lr: relative difference {rel:.3e}, bound {bound:.3e}"
        else:
            assert got[k] == want[k] and type(got[k]) is type(want[k]), (where, k, got[k], want[k])


@pytest.mark.parametrize("name", list(R.CASES))
def test_state_dicts_are_the_references(built_lib, golden, name):
    """4 + 5: state_dict() at steps 0, 14, 15 and 20 has the fixture's keys, counters and configuration, and its `_last_lr`
    (exact behind a warm-up and for the step schedule's closed form, within the recorded drift otherwise; the outer one stays
    at the last warm-up value); each of the fixture's dicts loads and the continuation is the uninterrupted sequence"""
    s, opt = _attached(name)
    assert s.base_lrs == list(R.BASE_LRS) and [g["lr"] for g in opt.param_groups] == list(R.BASE_LRS)
    restated = R.case(name)
    warm = R.CASES[name][1] > 0
    bound = 4 * float(golden[f"{name}/maxrel"])
    for e in R.DICT_STEPS:
        want = _dict(golden, name, e)
        s.set_last_epoch(e)
        _same_dict(s.state_dict(), want, warm, bound, f"{name}@{e}")
        fresh, fopt = _attached(name)
        before = json.dumps(sorted(want), sort_keys=True)
        fresh.load_state_dict(want)
        assert json.dumps(sorted(want), sort_keys=True) == before and ("after_scheduler" in want) == warm   # not consumed
        assert fresh.last_epoch == e
        seq = []
        for _ in range(R.STEPS - e):
            fopt.replayed()                            # the host mirror of one applying launch
            seq.append(fresh.get_last_lr())
        assert fresh.last_epoch == R.STEPS
        assert _bits(seq) == _bits([restated.lrs(k) for k in range(e + 1, R.STEPS + 1)])
    assert opt.staged == 1                             # the rows went to the device once, at construction


def test_load_state_dict_refuses_another_configuration(built_lib, golden):
    """6: a mismatching T_max, gamma, base_lrs (and the other configuration fields) raises and changes nothing"""
    s, _ = _attached("cosine_warm")
    good = _dict(golden, "cosine_warm", 15)
    s.set_last_epoch(3)
    for spoil in (dict(base_lrs=[0.002, 0.0002]), dict(multiplier=10), dict(warmup_epoch=7),
                  dict(after_scheduler=dict(good["after_scheduler"], T_max=71)),
                  dict(after_scheduler=dict(good["after_scheduler"], eta_min=0.0)),
                  dict(after_scheduler=dict(good["after_scheduler"], base_lrs=[0.1, 0.1])),
                  dict(after_scheduler=dict(good["after_scheduler"], last_epoch=5)), dict(last_epoch=-1)):
        with pytest.raises(ValueError, match="load_state_dict"):
            s.load_state_dict(dict(good, **spoil))
        assert s.last_epoch == 3
    with pytest.raises(ValueError, match="warm-up"):
        s.load_state_dict(_dict(golden, "cosine_cold", 15))
    with pytest.raises(ValueError, match="cosine"):
        s.load_state_dict(_dict(golden, "step_warm", 15))
    s.load_state_dict(good)
    assert s.last_epoch == 15
    m, _ = _attached("step_cold")
    good = _dict(golden, "step_cold", 20)
    for spoil in (dict(gamma=0.5), dict(milestones=Counter({49: 1, 71: 1})), dict(milestones=Counter({49: 2, 70: 1})),
                  dict(base_lrs=[0.002])):
        with pytest.raises(ValueError, match="load_state_dict"):
            m.load_state_dict(dict(good, **spoil))
    m.load_state_dict(good)
    assert m.last_epoch == 20 and m.get_last_lr() == list(R.BASE_LRS)


def test_optimizer_keeps_the_base_rates_the_device_was_given(built_lib):
    """param_groups[g]["lr"] is the base rate and stays it: a loaded optimiser state written under a host scheduler (its `lr`
    the rate of its step, its `initial_lr` the base) does not move it, another base rate is refused, and parameter groups
    cannot be added behind the schedule's back"""
    s, opt = _attached("cosine_warm")
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in R.BASE_LRS]
    theirs = torch.optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(ps, R.BASE_LRS)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = torch.optim.lr_scheduler.CosineAnnealingLR(theirs, T_max=70, eta_min=1e-6)
        for _ in range(5):
            theirs.step()
            host.step()
    state = theirs.state_dict()
    assert [g["lr"] for g in state["param_groups"]] != list(R.BASE_LRS)
    assert [g["initial_lr"] for g in state["param_groups"]] == list(R.BASE_LRS)
    opt.load_state_dict(state)
    assert [g["lr"] for g in opt.param_groups] == s.base_lrs == list(R.BASE_LRS)
    state["param_groups"][1]["initial_lr"] = 3e-4
    with pytest.raises(ValueError, match="base rate"):
        opt.load_state_dict(state)
    assert [g["lr"] for g in opt.param_groups] == list(R.BASE_LRS)
    with pytest.raises(NotImplementedError, match="fixed at construction"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})


def test_checkpoint_takes_the_schedule_as_its_scheduler(built_lib, tmp_path):
    import types
    import checkpoint
    s, opt = _attached("step_warm")
    s.set_last_epoch(17)
    net = torch.nn.Linear(2, 2)
    args = types.SimpleNamespace(log_dir=str(tmp_path), save_freq=1, checkpoint_path=None, start_epoch=0, ema=False)
    checkpoint.save_checkpoint(args, 1, net, opt, s, save_cur=True)
    saved = [f for f in os.listdir(tmp_path) if f.endswith(".pth")]
    assert saved
    s2, opt2 = _attached("step_warm")
    args.checkpoint_path = os.path.join(str(tmp_path), saved[0])
    checkpoint.load_checkpoint(args, net, opt2, s2, trust_pickle=True)
    assert s2.last_epoch == 17 and s2.state_dict() == s.state_dict()


def _declared_struct():
    """[(field, letter, count)] of `struct omnipq_lr_schedule` as include/omnipq_optim.h states it: this test's own reading"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(capi.INCLUDE, "omnipq_optim.h")).read(), flags=re.S)
    body = re.search(r"\bstruct\s+omnipq_lr_schedule\s*\{([^{}]*)\}\s*;", text).group(1)
    letters = {"int": "i", "long long": "l", "double": "d"}
    out = []
    for stmt in body.split(";"):
        if stmt.strip():
            m = re.fullmatch(r"\s*(int|long long|double)\s+(\w+)(?:\[(\d+)\])?\s*", stmt)
            out.append((m.group(2), letters[m.group(1)], int(m.group(3)) if m.group(3) else None))
    return out


def test_struct_and_entry_points_are_declared_exported_and_reported(built_lib):
    """7a: the record text of struct omnipq_lr_schedule is the header's, and the ctypes structure built from it has the layout
    the compiler was held to; the new entry points carry the signatures the header declares"""
    layout = _declared_struct()
    assert [f for f, _, _ in layout] == ["kind", "n_milestones", "warmup_iters", "t_max", "multiplier", "eta_min", "milestones",
                                         "gamma_pow"]
    want = "struct omnipq_lr_schedule " + " ".join(f"{f}:{t}" + (f"*{n}" if n else "") for f, t, n in layout)
    declared = capi.declared_signatures()
    assert declared["omnipq_adamw_sched_finalize"] == FINALIZE
    assert declared["omnipq_lr_schedule_eval"] == ("i", "ippppp")
    assert declared["omnipq_lr_schedule_record"] == ("s", "") and declared["omnipq_lr_schedule_max_milestones"] == ("i", "")
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        for name in ("omnipq_adamw_sched_finalize", "omnipq_lr_schedule_eval", "omnipq_lr_schedule_record",
                     "omnipq_lr_schedule_max_milestones"):
            assert hasattr(lib, name) and got[name] == declared[name], (path, name)
        lib.omnipq_lr_schedule_record.restype = ctypes.c_char_p
        assert lib.omnipq_lr_schedule_record().decode() == want, path
        assert lib.omnipq_lr_schedule_max_milestones() == dict((f, n) for f, _, n in layout)["milestones"] == 8
        assert lib.omnipq_abi_version() == 5                      # an addition only
    import build as omnipq_build
    assert omnipq_build.plain_struct_record("omnipq_lr_schedule") == want
    assert "static_assert(sizeof(omnipq_lr_schedule) == 176" in omnipq_build.plain_struct_text()
    import pointnet2_utils
    rec = pointnet2_utils._load_ext().lr_schedule_struct()
    assert issubclass(rec, ctypes.Structure) and ctypes.sizeof(rec) == 176
    ctype = {"i": ctypes.c_int, "l": ctypes.c_longlong, "d": ctypes.c_double}
    assert rec._fields_ == [(f, ctype[t] * n if n else ctype[t]) for f, t, n in layout]
    assert [getattr(rec, f).offset for f, _, _ in layout] == [0, 4, 8, 16, 24, 32, 40, 104]
    # the host copy the binding uploads
    import optim
    s = optim.LRSchedule("step", 7, 12, 2, 100, (6, 9), 0.1)._struct()
    assert (s.kind, s.n_milestones, s.warmup_iters, s.t_max, s.multiplier, s.eta_min) == (1, 2, 14, 70, 100.0, 1e-6)
    assert list(s.milestones) == [28, 49, 0, 0, 0, 0, 0, 0] and list(s.gamma_pow) == [0.1 ** j for j in range(9)]


def test_malformed_calls_return_einval_without_a_gpu(built_lib):
    """7b: every OMNIPQ_EINVAL of omnipq_lr_schedule_eval and omnipq_adamw_sched_finalize, nothing launched"""
    import pointnet2_utils
    lib = pointnet2_utils._load_ext()._lib0
    p, null = ctypes.c_void_p(0x1000), None                      # "some non-null pointer": validation comes first

    def ev(ngroups=2, sched=p, base_lr=p, state=p, lr_now=p):
        return lib.omnipq_lr_schedule_eval(ngroups, sched, base_lr, state, lr_now, None)

    for bad in (dict(ngroups=0), dict(ngroups=-1), dict(sched=null), dict(base_lr=null), dict(state=null), dict(lr_now=null)):
        assert ev(**bad) == EINVAL, bad

    def fin(nchunks=4, partials=p, hyper=p, ngroups=2, accum_steps=1, counters=p, accum=null, ema_state=null, ema_coef=null,
            scaler_cfg=null, scaler_state=null, sched=p, base_lr=p, state=p, lr_now=p, result=p, coef=p):
        return lib.omnipq_adamw_sched_finalize(nchunks, partials, hyper, ngroups, accum_steps, counters, accum, ema_state,
                                               ema_coef, scaler_cfg, scaler_state, sched, base_lr, state, lr_now, result, coef,
                                               None)

    for bad in (dict(state=null), dict(sched=null), dict(base_lr=null), dict(lr_now=null),       # a schedule in part
                dict(sched=null, base_lr=null), dict(sched=null, base_lr=null, state=null),
                dict(scaler_cfg=p), dict(scaler_state=p),                                        # half a scaler
                dict(ema_state=p), dict(ema_coef=p),                                             # half a teacher
                dict(accum_steps=3), dict(accum_steps=2, ema_state=p, ema_coef=p),               # micro-batches without their counter
                dict(accum_steps=0), dict(accum_steps=0, accum=p), dict(accum_steps=-1, accum=p),
                dict(nchunks=-1), dict(partials=null), dict(hyper=null), dict(ngroups=0), dict(counters=null),
                dict(result=null), dict(coef=null)):
        assert fin(**bad) == EINVAL, bad
