"""Mean-teacher weight averaging inside FusedAdamW's launches (optim.FusedAdamW.attach_teacher, CapturedStep(ema_in_step=True);
include/omnipq_optim.h: omnipq_adamw_ema_*) without a GPU: the entry points exist and validate their arguments on the host,
what is accepted and refused, the rounding contract of the two coefficients, and the decay's place in the staged rows."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import capi
from test_fused_adamw_host import _Small, _groups, _same_structure, _two_torch_steps

ENTRY_POINTS = {"omnipq_adamw_check_ema_table": ("i", "ipipipi"),
                "omnipq_adamw_ema_finalize": ("i", "ippiippppppp"),
                "omnipq_adamw_ema_update": ("i", "iipppiiippppppppp")}
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


def test_malformed_calls_return_einval_without_a_gpu(built_lib):
    import pointnet2_utils
    lib = pointnet2_utils._load_ext()._lib0
    p, null = ctypes.c_void_p(0x1000), None                      # "some non-null pointer": validation comes first
    fin = lib.omnipq_adamw_ema_finalize       # nchunks, partials, hyper, ngroups, accum_steps, counters, accum, ema_state,
    #                                           result, coef, ema_coef
    assert fin(-1, p, p, 2, 1, p, null, p, p, p, p, None) == EINVAL
    assert fin(4, null, p, 2, 1, p, null, p, p, p, p, None) == EINVAL
    assert fin(4, p, null, 2, 1, p, null, p, p, p, p, None) == EINVAL
    assert fin(4, p, p, 0, 1, p, null, p, p, p, p, None) == EINVAL
    assert fin(4, p, p, 2, 0, p, p, p, p, p, p, None) == EINVAL
    assert fin(4, p, p, 2, 3, p, null, p, p, p, p, None) == EINVAL           # three micro-batches without their counter
    assert fin(4, p, p, 2, 1, null, null, p, p, p, p, None) == EINVAL
    assert fin(4, p, p, 2, 1, p, null, null, p, p, p, None) == EINVAL        # no ema_state
    assert fin(4, p, p, 2, 1, p, null, p, null, p, p, None) == EINVAL
    assert fin(4, p, p, 2, 1, p, null, p, p, null, p, None) == EINVAL
    assert fin(4, p, p, 2, 1, p, null, p, p, p, null, None) == EINVAL        # no ema_coef
    up = lib.omnipq_adamw_ema_update          # nrec, nchunks, records, ema_ptrs, chunks, chunk, n_only, n_only_chunks, ema_only,
    #                                           only_chunks, exp_avg, acc, accum, coef, ema_coef, result

    def call(nrec=2, nchunks=4, records=p, ema_ptrs=p, chunks=p, chunk=4096, n_only=1, n_only_chunks=1, ema_only=p,
             only_chunks=p, exp_avg=null, acc=null, accum=null, coef=p, ema_coef=p, result=p):
        return up(nrec, nchunks, records, ema_ptrs, chunks, chunk, n_only, n_only_chunks, ema_only, only_chunks, exp_avg, acc,
                  accum, coef, ema_coef, result, None)

    for bad in (dict(records=null), dict(ema_ptrs=null), dict(chunks=null), dict(coef=null), dict(ema_coef=null),
                dict(result=null),                                                       # null tables
                dict(nrec=-2), dict(nchunks=-4), dict(n_only=-1), dict(n_only_chunks=-1),  # negative counts
                dict(chunk=4097), dict(chunk=0),
                dict(ema_only=null), dict(only_chunks=null),                              # n_only > 0 without its tables
                dict(accum=p, exp_avg=null, acc=p), dict(accum=p, exp_avg=p, acc=null),    # accumulating without a base
                dict(nrec=0), dict(n_only=0)):                                             # chunks of records that do not exist
        assert call(**bad) == EINVAL, bad
    assert call(nrec=0, nchunks=0, records=null, ema_ptrs=null, chunks=null, n_only=0, n_only_chunks=0, ema_only=null,
                only_chunks=null) == 0                                                    # nothing to do


def test_check_ema_table_accepts_a_good_host_table_and_refuses_each_bad_one(built_lib):
    import optim
    import pointnet2_utils
    lib = pointnet2_utils._load_ext()._lib0
    assert optim.EMA_ONLY.itemsize == 24

    def check(ptrs, only, chunks, chunk=4096):
        ptrs = np.asarray(ptrs, dtype=np.uint64)
        rec = np.zeros(len(only), dtype=optim.EMA_ONLY)
        for i, o in enumerate(only):
            rec[i] = o
        chunks = np.asarray(chunks, dtype=np.int32).reshape(-1, 2)
        return lib.omnipq_adamw_check_ema_table(len(ptrs), ptrs.ctypes.data_as(ctypes.c_void_p), len(rec),
                                                rec.ctypes.data_as(ctypes.c_void_p), len(chunks),
                                                chunks.ctypes.data_as(ctypes.c_void_p), chunk)

    ptrs, only, chunks = [0x1000, 0x2004], [(0x3000, 0x4000, 5000), (0x5008, 0x600c, 1)], [(0, 0), (0, 1), (1, 0)]
    assert check(ptrs, only, chunks) == 0
    assert check(ptrs, [], []) == 0 and check([], only, chunks) == 0
    assert check([0x1000, 0], only, chunks) == EINVAL                     # a null teacher pointer
    assert check([0x1000, 0x2002], only, chunks) == EINVAL                # ... one that is not 4-byte aligned
    assert check(ptrs, [(0, 0x4000, 5000)], [(0, 0)]) == EINVAL           # an ema_only record with a null pointer
    assert check(ptrs, [(0x3000, 0, 5000)], [(0, 0)]) == EINVAL
    assert check(ptrs, [(0x3000, 0x4000, -1)], []) == EINVAL              # ... with a negative numel
    assert check(ptrs, [(0x3002, 0x4000, 5000)], [(0, 0)]) == EINVAL
    assert check(ptrs, only, chunks + [(0, 2)]) == EINVAL                 # 2 * 4096 >= 5000: past its record
    assert check(ptrs, only, chunks + [(1, 1)]) == EINVAL
    assert check(ptrs, only, chunks + [(2, 0)]) == EINVAL                 # no such record
    assert check(ptrs, only, chunks + [(0, -1)]) == EINVAL
    assert check(ptrs, only, chunks, chunk=1000) == EINVAL
    assert lib.omnipq_adamw_check_ema_table(2, None, 0, None, 0, None, 4096) == EINVAL
    assert lib.omnipq_adamw_check_ema_table(0, None, 1, None, 0, None, 4096) == EINVAL
    assert lib.omnipq_adamw_check_ema_table(-1, None, 0, None, 0, None, 4096) == EINVAL


def _pair():
    torch.manual_seed(0)
    net = _Small()
    teacher = copy.deepcopy(net)
    for p in teacher.parameters():
        p.requires_grad_(False)
    return net, teacher


def test_attach_teacher_refuses_what_it_cannot_average(built_lib):
    import optim
    net, teacher = _pair()
    fused = optim.FusedAdamW(_groups(net), lr=2e-3)
    assert fused.global_step is None and fused.ema_decay == 0.0
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            fused.attach_teacher(net, teacher, bad)
    # a teacher tensor that is not contiguous f32 of its partner's shape
    for spoil in (lambda p: p.data.double(), lambda p: torch.zeros(p.numel() + 1), lambda p: torch.zeros(*p.shape, 2)[..., 0]):
        t2 = copy.deepcopy(teacher)
        first = next(t2.parameters())
        first.data = spoil(first)
        assert first.dtype != torch.float32 or first.shape != next(net.parameters()).shape or not first.is_contiguous()
        with pytest.raises(ValueError, match="teacher parameter"):
            fused.attach_teacher(net, t2, 0.999)
    # ... or is on another device
    t3 = copy.deepcopy(teacher)
    t3.backbone.weight = torch.nn.Parameter(torch.zeros_like(t3.backbone.weight, device="meta"), requires_grad=False)
    with pytest.raises(ValueError, match="teacher parameter"):
        fused.attach_teacher(net, t3, 0.999)
    # a student parameter the optimiser does not own
    partial = optim.FusedAdamW([{"params": list(net.backbone.parameters())}], lr=2e-3)
    with pytest.raises(ValueError, match="does not own"):
        partial.attach_teacher(net, teacher, 0.999)
    with pytest.raises(ValueError, match="parameters"):
        fused.attach_teacher(net, teacher.backbone, 0.999)
    for bad in (-1, 1.0, True):
        with pytest.raises(ValueError, match="global_step"):
            fused.attach_teacher(net, teacher, 0.999, global_step=bad)
    assert fused.global_step is None                               # a refused call attached nothing
    with pytest.raises(RuntimeError, match="no teacher"):
        fused.set_global_step(3)
    # accepted: the default first step is the reference's first `I`
    fused.attach_teacher(net, teacher, 0.999)
    assert fused.global_step == 1 and fused.ema_decay == 0.999
    assert fused.ema_state.dtype == torch.int64 and tuple(fused.ema_state.shape) == (1,)
    assert fused.ema_coef.dtype == torch.float32 and tuple(fused.ema_coef.shape) == (2,)
    fused.set_global_step(41)
    assert fused.global_step == 41
    with pytest.raises(ValueError, match=">= 0"):
        fused.set_global_step(-1)
    # snapshot / restore carry the global step, the coefficients and the teacher's weights
    saved = fused.snapshot()
    t0 = [p.detach().clone() for p in teacher.parameters()]
    fused.set_global_step(45)
    with torch.no_grad():
        for p in teacher.parameters():
            p.add_(1.0)
    fused.restore(saved)
    assert fused.global_step == 41
    for p, q in zip(teacher.parameters(), t0):
        assert torch.equal(p, q)
    # state_dict() is still torch.optim.AdamW's
    want = _two_torch_steps(net).state_dict()
    fused.load_state_dict(want)
    _same_structure(fused.state_dict(), want)
    assert fused.global_step == 41                                 # not optimiser state: a loaded state leaves it alone
    fused.detach_teacher()
    assert fused.global_step is None and fused.ema_decay == 0.0 and fused.staging[2, 2].item() == 0.0
    with pytest.raises(RuntimeError, match="attached or detached"):
        fused.restore(saved)


def test_captured_step_takes_ema_in_step_only_with_teacher_decay_and_fused_adamw(built_lib):
    import optim
    import train_step
    net, teacher = _pair()

    def build(**kw):
        return train_step.CapturedStep(net, lambda ep, lab: ep, torch.zeros(1, 4, 3), graph=False, prefetch=None, **kw)

    def fused():
        return optim.FusedAdamW(_groups(net), lr=2e-3)

    for kw in (dict(teacher=teacher, ema=0.999),                                   # no FusedAdamW
               dict(optimizer=fused(), ema=0.999),                                 # no teacher
               dict(optimizer=fused(), teacher=teacher),                           # no decay
               dict(optimizer=fused(), teacher=teacher, ema=True)):
        with pytest.raises(ValueError, match="ema_in_step"):
            build(ema_in_step=True, **kw)
    opt = fused()
    st = build(optimizer=opt, teacher=teacher, ema=0.999, ema_in_step=True)
    assert st.ema_in_step is True and opt.global_step == 1 and opt.ema_decay == 0.999
    with pytest.raises(RuntimeError, match="ema_in_step"):
        st.update_teacher(1)
    # the default changes nothing: no teacher is attached, update_teacher() is the separate launch it was
    opt2 = fused()
    st2 = build(optimizer=opt2, teacher=teacher, ema=0.999)
    assert st2.ema_in_step is False and opt2.global_step is None
    with pytest.raises(RuntimeError, match="CPU not supported"):
        st2.update_teacher(1)


def test_coefficients_round_like_the_arguments_of_the_separate_launch():
    """(alpha, beta) as the finalise launch forms them (include/omnipq_optim.h), restated in numpy: f64, then one rounding to
    f32 each -- against the Python doubles of ema.ema_alpha as they reach omnipq_ema_update's float parameters."""
    import ema
    for d in (0.0, 0.5, 0.75, 0.999, 1.0):
        for g in range(0, 2001):
            a = np.fmin(np.float64(1.0) - np.float64(1.0) / np.float64(np.int64(g) + 1), np.float64(d))
            alpha, beta = np.float32(a), np.float32(np.float64(1.0) - a)
            want = ema.ema_alpha(d, g)
            assert alpha == np.float32(want) and beta == np.float32(1.0 - want), (d, g)
            assert alpha.tobytes() == np.float32(want).tobytes() and beta.tobytes() == np.float32(1.0 - want).tobytes()
    assert np.float32(ema.ema_alpha(0.75, 0)) == 0.0 and ema.ema_alpha(0.75, 3) == 0.75 == 1.0 - 1.0 / 4        # the tie


def test_rows_carry_the_decay_in_slot_2_of_the_last_row(built_lib):
    import optim
    net, teacher = _pair()
    fused = optim.FusedAdamW(_groups(net), lr=2e-3, max_norm=0.1, grad_scale=0.5)
    assert fused._rows()[-1].tolist() == [0.1, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]           # zero today
    fused.attach_teacher(net, teacher, 0.999)
    assert fused._rows()[-1].tolist() == [0.1, 0.5, 0.999, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert fused.staging[2, :3].tolist() == [0.1, 0.5, 0.999]                               # attach_teacher staged it
    assert (fused._rows()[:-1, 5:] == 0).all()
    assert fused.sync_hyperparameters() is False
    fused.ema_decay = 0.99
    assert fused.sync_hyperparameters() is True and fused.staging[2, 2].item() == 0.99
    assert fused.sync_hyperparameters() is False
