"""GPU: the whole model, one forward + backward (batch 2, 8192 points, bf16, dropout on, the same dropout seed) with the
prediction heads' backward grouped over all stages (pred_heads._HEADS_BWD_GROUP) and per stage: every `end_points` entry
and every parameter gradient bit-equal, and the C-ABI calls made (pointnet2/_ext.py: set_timing_sink) show which route ran."""
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_once(net, pc, on, only=None):
    """only: prefixes of the stages whose outputs reach the loss (None: every end_points entry, as bench.py's loss)"""
    import bench
    import dropout_state
    import pred_heads
    import sa_fused
    before = pred_heads._HEADS_BWD_GROUP
    calls = []
    try:
        pred_heads._HEADS_BWD_GROUP = on
        dropout_state.STATE.set_state(torch.device(DEV), 0x5EED5EED)
        net.zero_grad(set_to_none=True)
        sa_fused._ext.set_timing_sink(calls)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ep = net({"point_clouds": pc})
            loss = bench.loss_of(ep if only is None else {k: v for k, v in ep.items() if k.startswith(only)})
        with sa_fused.deferred_wgrads():
            loss.backward()
        torch.cuda.synchronize()
    finally:
        sa_fused._ext.set_timing_sink(None)
        pred_heads._HEADS_BWD_GROUP = before
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}
    return {k: v.detach().clone() for k, v in ep.items()}, grads, loss.detach().clone(), [(n, a) for n, a, _, _ in calls]


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t.view(torch.int32) if t.dtype is torch.float32 else t


def count(calls, name):
    return sum(1 for n, _ in calls if n == name)


def same(on, off):
    ep_on, g_on, loss_on, _ = on
    ep_off, g_off, loss_off, _ = off
    assert list(ep_on) == list(ep_off) and len(ep_on) >= 119
    for k in ep_on:
        assert ep_on[k].dtype == ep_off[k].dtype and ep_on[k].requires_grad == ep_off[k].requires_grad, k
        assert torch.equal(bits(ep_on[k]), bits(ep_off[k])), k
    n_grads = 0
    for k in g_on:
        assert (g_on[k] is None) == (g_off[k] is None), k
        if g_on[k] is not None:
            assert torch.equal(bits(g_on[k]), bits(g_off[k])), k
            n_grads += 1
    return n_grads


@pytest.fixture(scope="module")
def model():
    import bench
    import synth
    from procedural import load_procedural
    pc = synth.make_clouds(90, 2, 8192, kind="room").to(DEV)
    net = load_procedural(bench.build_model(0)).to(DEV).train()
    run_once(net, pc, False)          # the first pass over fresh parameters prepares weights and plans: not part of any comparison
    return net, pc


def test_whole_model_is_bit_equal_with_the_heads_backward_grouped_and_per_stage(model):
    import pred_heads
    net, pc = model
    assert pred_heads._HEADS_BWD_GROUP is True                                   # the default ships on
    stages = len(net.decoder) + 1
    off = run_once(net, pc, False)
    on = run_once(net, pc, True)
    assert same(on, off) >= 300
    calls_on, calls_off = on[3], off[3]
    assert count(calls_off, "omnipq_decode_pair_bwd") == stages == 7 and count(calls_off, "omnipq_decode_pair_group_bwd") == 0
    assert count(calls_on, "omnipq_decode_pair_bwd") == 0 and 1 <= count(calls_on, "omnipq_decode_pair_group_bwd") <= 2
    # the forward is what it was, and the same problems run in backward: the calls differ in the decode backward alone
    import collections
    skip = ("omnipq_decode_pair_group_bwd", "omnipq_decode_pair_bwd")
    n_on = collections.Counter(repr(c) for c in calls_on if c[0] not in skip)
    n_off = collections.Counter(repr(c) for c in calls_off if c[0] not in skip)
    assert n_on == n_off, (sorted((n_on - n_off).items()), sorted((n_off - n_on).items()))
    for name in ("omnipq_decode_pair", "omnipq_decode_pair_pos16", "omnipq_gemm_nt_e16_stats"):
        assert count(calls_on, name) == count(calls_off, name) > 0, name


def test_stages_without_gradient_are_left_out_of_the_group(model):
    """the loss reads two stages' outputs only: the other stages' backward programs do not run, on either route"""
    net, pc = model
    only = ("2head_", "last_")
    off = run_once(net, pc, False, only)
    on = run_once(net, pc, True, only)
    assert same(on, off) >= 100
    calls_on, calls_off = on[3], off[3]
    assert count(calls_off, "omnipq_decode_pair_bwd") == 2
    assert count(calls_on, "omnipq_decode_pair_bwd") == 0 and count(calls_on, "omnipq_decode_pair_group_bwd") == 1
    for name in ("omnipq_bn_bwd_apply_fused", "omnipq_gemm_nt_e16_bnbwd"):
        assert count(calls_on, name) == count(calls_off, name) > 0, name
