"""GPU: the whole model, one forward + backward (batch 2, 8192 points, bf16, dropout on, the same dropout seed) with the
stage-boundary folds on and off: every `end_points` entry and every parameter gradient bit-equal, and the C-ABI calls made
(pointnet2/_ext.py: set_timing_sink) show that the folds are what ran -- no omnipq_split_rows / omnipq_merge_rows, no
omnipq_pad_rows_e16 of the query positions; the key positions' one conversion stays."""
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = (("decoder_rows", "LN_SPLIT"), ("pred_heads", "_POS_ROWS16"), ("pq_transformer", "_JOIN_ROWS"))


def run_once(net, pc, on):
    import importlib
    import bench
    import dropout_state
    import sa_fused
    mods = {m: importlib.import_module(m) for m, _ in SWITCHES}
    before = {(m, n): getattr(mods[m], n) for m, n in SWITCHES if hasattr(mods[m], n)}
    calls = []
    try:
        for m, n in before:
            setattr(mods[m], n, on)
        dropout_state.STATE.set_state(torch.device(DEV), 0x5EED5EED)
        net.zero_grad(set_to_none=True)
        sa_fused._ext.set_timing_sink(calls)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ep = net({"point_clouds": pc})
            loss = bench.loss_of(ep)
        with sa_fused.deferred_wgrads():
            loss.backward()
        torch.cuda.synchronize()
    finally:
        sa_fused._ext.set_timing_sink(None)
        for (m, n), v in before.items():
            setattr(mods[m], n, v)
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}
    return {k: v.detach().clone() for k, v in ep.items()}, grads, loss.detach().clone(), [(n, a) for n, a, _, _ in calls]


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t.view(torch.int32) if t.dtype is torch.float32 else t


def test_whole_model_is_bit_equal_with_the_boundary_folds_on_and_off():
    import bench
    import decoder_rows
    import pq_transformer
    import pred_heads
    import synth
    from procedural import load_procedural
    assert decoder_rows.LN_SPLIT is True and pred_heads._POS_ROWS16 is True          # the defaults ship on
    B, P = 2, 256 + 256
    pc = synth.make_clouds(90, B, 8192, kind="room").to(DEV)
    net = load_procedural(bench.build_model(0)).to(DEV).train()
    n_layers = len(net.decoder)
    ep_off, g_off, loss_off, calls_off = run_once(net, pc, False)
    ep_on, g_on, loss_on, calls_on = run_once(net, pc, True)
    assert sorted(ep_on) == sorted(ep_off) and len(ep_on) >= 119
    for k in sorted(ep_on):
        assert ep_on[k].dtype == ep_off[k].dtype and torch.equal(bits(ep_on[k]), bits(ep_off[k])), k
    n_grads = 0
    for k in g_on:
        assert (g_on[k] is None) == (g_off[k] is None), k
        if g_on[k] is not None:
            assert torch.equal(bits(g_on[k]), bits(g_off[k])), k
            n_grads += 1
    assert n_grads >= 300

    def count(calls, name, pred=lambda a: True):
        return sum(1 for n, a in calls if n == name and pred(a))

    def query_pos(a):            # omnipq_pad_rows_e16(n, cin, k, ldx, ..., x_is_f32): the joint query positions of a stage
        return a[0] == B * P and a[1] == 3

    def key_pos(a):
        return a[0] == B * 1024 and a[1] == 3

    # off: one split and one merge per stage, one conversion of the query positions per layer; on: none of them
    assert count(calls_off, "omnipq_split_rows") == n_layers and count(calls_off, "omnipq_merge_rows") == n_layers
    assert count(calls_off, "omnipq_pad_rows_e16", query_pos) == n_layers
    assert count(calls_on, "omnipq_split_rows") == 0 and count(calls_on, "omnipq_merge_rows") == 0
    assert count(calls_on, "omnipq_pad_rows_e16", query_pos) == 0
    assert count(calls_on, "omnipq_pad_rows_e16", key_pos) == count(calls_off, "omnipq_pad_rows_e16", key_pos) == 1
    assert count(calls_on, "omnipq_add_dropout_layernorm_split") == n_layers
    assert count(calls_on, "omnipq_add_dropout_layernorm_bwd_partials_split") + \
        count(calls_on, "omnipq_add_dropout_layernorm_bwd_split") == n_layers
    assert count(calls_on, "omnipq_decode_pair_pos16") == n_layers and count(calls_off, "omnipq_decode_pair_pos16") == 0
    assert count(calls_on, "omnipq_decode_pair") == 1 and count(calls_off, "omnipq_decode_pair") == n_layers + 1
    if hasattr(pq_transformer, "_JOIN_ROWS"):
        assert count(calls_on, "omnipq_merge_rows_f32") == 1 and count(calls_on, "omnipq_split_rows_sum") == 1
        assert count(calls_off, "omnipq_merge_rows_f32") == 0 and count(calls_off, "omnipq_split_rows_sum") == 0
