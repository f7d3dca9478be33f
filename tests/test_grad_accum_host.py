"""Gradient accumulation (FusedAdamW(accum_steps=k), CapturedStep(step_freq=k); include/omnipq_optim.h: omnipq_adamw_accum_*)
without a GPU: the entry points exist and validate their arguments on the host, what is accepted and refused, and the
state_dict of an accumulating optimiser is still torch.optim.AdamW's."""
import ctypes

import pytest
import torch

import capi
from test_fused_adamw_host import _Small, _groups, _same_structure, _two_torch_steps

ENTRY_POINTS = {"omnipq_adamw_accum_sqnorm": ("i", "iippipippppp"),
                "omnipq_adamw_accum_finalize": ("i", "ippiippppp"),
                "omnipq_adamw_accum_update": ("i", "iippipppppp")}
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
    import pointnet2_utils
    assert pointnet2_utils._ext.ABI_VERSION == 5


def test_malformed_calls_return_einval_without_a_gpu(built_lib):
    import pointnet2_utils
    lib = pointnet2_utils._load_ext()._lib0
    p, null = ctypes.c_void_p(0x1000), None                      # "some non-null pointer": validation comes first
    sq = lib.omnipq_adamw_accum_sqnorm        # nrec, nchunks, records, chunks, chunk, hyper, ngroups, exp_avg, acc, accum, partials
    assert sq(2, 4, null, p, 4096, p, 2, p, p, p, p, None) == EINVAL
    assert sq(2, 4, p, null, 4096, p, 2, p, p, p, p, None) == EINVAL
    assert sq(2, 4, p, p, 4096, null, 2, p, p, p, p, None) == EINVAL
    assert sq(2, 4, p, p, 4096, p, 2, null, p, p, p, None) == EINVAL
    assert sq(2, 4, p, p, 4096, p, 2, p, null, p, p, None) == EINVAL
    assert sq(2, 4, p, p, 4096, p, 2, p, p, null, p, None) == EINVAL
    assert sq(2, 4, p, p, 4096, p, 2, p, p, p, null, None) == EINVAL
    assert sq(-1, 4, p, p, 4096, p, 2, p, p, p, p, None) == EINVAL
    assert sq(2, -4, p, p, 4096, p, 2, p, p, p, p, None) == EINVAL
    assert sq(2, 4, p, p, 4096, p, 0, p, p, p, p, None) == EINVAL
    assert sq(2, 4, p, p, 1000, p, 2, p, p, p, p, None) == EINVAL
    assert sq(2, 4, p, p, 0, p, 2, p, p, p, p, None) == EINVAL
    assert sq(0, 0, null, null, 4096, p, 2, p, p, p, null, None) == 0          # nothing to do
    fin = lib.omnipq_adamw_accum_finalize     # nchunks, partials, hyper, ngroups, accum_steps, counters, accum, result, coef
    assert fin(-1, p, p, 2, 3, p, p, p, p, None) == EINVAL
    assert fin(4, null, p, 2, 3, p, p, p, p, None) == EINVAL
    assert fin(4, p, null, 2, 3, p, p, p, p, None) == EINVAL
    assert fin(4, p, p, 0, 3, p, p, p, p, None) == EINVAL
    assert fin(4, p, p, 2, 0, p, p, p, p, None) == EINVAL
    assert fin(4, p, p, 2, -2, p, p, p, p, None) == EINVAL
    assert fin(4, p, p, 2, 3, null, p, p, p, None) == EINVAL
    assert fin(4, p, p, 2, 3, p, null, p, p, None) == EINVAL
    assert fin(4, p, p, 2, 3, p, p, null, p, None) == EINVAL
    assert fin(4, p, p, 2, 3, p, p, p, null, None) == EINVAL
    up = lib.omnipq_adamw_accum_update        # nrec, nchunks, records, chunks, chunk, exp_avg, acc, accum, coef, result
    assert up(2, 4, null, p, 4096, p, p, p, p, p, None) == EINVAL
    assert up(2, 4, p, null, 4096, p, p, p, p, p, None) == EINVAL
    assert up(2, 4, p, p, 4096, null, p, p, p, p, None) == EINVAL
    assert up(2, 4, p, p, 4096, p, null, p, p, p, None) == EINVAL
    assert up(2, 4, p, p, 4096, p, p, null, p, p, None) == EINVAL
    assert up(2, 4, p, p, 4096, p, p, p, null, p, None) == EINVAL
    assert up(2, 4, p, p, 4096, p, p, p, p, null, None) == EINVAL
    assert up(-2, 4, p, p, 4096, p, p, p, p, p, None) == EINVAL
    assert up(2, -4, p, p, 4096, p, p, p, p, p, None) == EINVAL
    assert up(2, 4, p, p, 4097, p, p, p, p, p, None) == EINVAL
    assert up(0, 0, null, null, 4096, p, p, p, p, p, None) == 0


def test_accum_steps_is_validated_and_mirrored_on_the_host(built_lib):
    import optim
    torch.manual_seed(0)
    net = _Small()
    for bad in (0, -1, 2.0, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="accum_steps"):
            optim.FusedAdamW(_groups(net), lr=2e-3, accum_steps=bad)
    one = optim.FusedAdamW(_groups(net), lr=2e-3)
    assert one.accum_steps == 1 and one.acc is None and one.accum is None          # the default allocates nothing new
    assert one.micro == 0 and one.is_update_step is False
    one.reset_accumulation()                                                       # a no-op, not an error
    three = optim.FusedAdamW(_groups(net), lr=2e-3, accum_steps=3)
    assert three.accum_steps == 3 and three.micro == 0 and three.is_update_step is False
    # the accumulator is laid out exactly like exp_avg; {micro, apply} is two device words
    assert three.acc.shape == three.exp_avg.shape and three.acc.dtype == torch.float32
    assert three.accum.dtype == torch.int64 and three.accum.tolist() == [0, 0]
    # the mirror a replayed launch advances: applying on every third call
    seen = []
    for _ in range(7):
        three.replayed()
        seen.append((three.micro, three.is_update_step))
    assert seen == [(1, False), (2, False), (0, True), (1, False), (2, False), (0, True), (1, False)]
    # snapshot / restore carry the counter and its mirror (CapturedStep's warm-up runs advance both)
    saved = three.snapshot()
    three.accum[0] = 2
    three.replayed()
    assert three.micro == 2
    three.restore(saved)
    assert three.micro == 1 and three.is_update_step is False and three.accum.tolist() == [0, 0]
    three.accum[0] = 1
    three.reset_accumulation()
    assert three.micro == 0 and three.accum.tolist() == [0, 0]


def test_captured_step_accepts_step_freq_only_with_a_matching_optimizer(built_lib):
    import optim
    import train_step
    torch.manual_seed(0)
    net = _Small()

    def build(**kw):
        return train_step.CapturedStep(net, lambda ep, lab: ep, torch.zeros(1, 4, 3), graph=False, prefetch=None, **kw)

    def fused(k):
        return optim.FusedAdamW(_groups(net), lr=2e-3, accum_steps=k)

    refused = [dict(step_freq=2), dict(step_freq=2, optimizer=fused(1)), dict(step_freq=2, optimizer=fused(3)),
               dict(step_freq=1, optimizer=fused(2)), dict(step_freq=0), dict(step_freq=3, optimizer=fused(2))]
    for kw in refused:
        with pytest.raises(ValueError, match="accumulation") as err:
            build(**kw)
        assert "FusedAdamW(accum_steps=" in str(err.value), kw
    for k in (1, 2, 3):
        opt = fused(k)
        st = build(step_freq=k, optimizer=opt)
        assert st.optimizer is opt and st.step_freq == k and st.is_update_step is False and opt.micro == 0
    assert build().step_freq == 1                                  # no optimizer, no accumulation: as before
    with pytest.raises(TypeError, match="FusedAdamW"):
        build(step_freq=2, optimizer=torch.optim.AdamW(net.parameters()))


def test_state_dict_of_an_accumulating_optimizer_is_torch_adamws(built_lib):
    import optim
    torch.manual_seed(0)
    net = _Small()
    want = _two_torch_steps(net).state_dict()
    fused = optim.FusedAdamW(_groups(net), lr=1.0, weight_decay=0.0, accum_steps=3)
    fused.replayed()                                               # as if one micro-batch had been summed
    assert fused.micro == 1
    fused.load_state_dict(want)
    assert fused.micro == 0 and fused.accum.tolist() == [0, 0]     # a loaded state starts a fresh accumulation
    assert fused.t == 2 and fused.skipped == 0 and fused.accum_steps == 3
    got = fused.state_dict()
    _same_structure(got, want)                                     # torch's keys only: the accumulator is not saved
    back = torch.optim.AdamW(_groups(net), lr=1.0)
    back.load_state_dict(got)
    _same_structure(back.state_dict(), want)
    again = optim.FusedAdamW(_groups(net), lr=1.0, accum_steps=1)  # ... and an accum_steps=1 optimiser reads it as well
    again.load_state_dict(got)
    _same_structure(again.state_dict(), want)
    fresh = optim.FusedAdamW(_groups(net), lr=2e-3, weight_decay=5e-4, accum_steps=3).state_dict()
    ref = torch.optim.AdamW(_groups(net), lr=2e-3, weight_decay=5e-4).state_dict()
    assert fresh["state"] == {} == ref["state"]
    for ga, gb in zip(fresh["param_groups"], ref["param_groups"]):
        assert ga == gb
