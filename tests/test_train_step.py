"""omni-pq_amd/train_step.py: the captured training step as a product API.

CPU: the look-ahead iterator and the argument contract.  GPU: a replayed `CapturedStep` equals the same steps launched
eagerly -- forward outputs and the loss bit for bit, gradients to the run-to-run noise of the backward pass -- whether the
batches are announced one call ahead (the fast path: sampling chain of the next batch underneath the running step) or not.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in ("omni-pq_amd", "omni-pq_amd/pointnet2", "omni-pq_amd/models"):
    sys.path.insert(0, os.path.join(REPO, p))
sys.path.insert(0, HERE)


def test_lookahead_pairs_every_item_with_its_successor(built_lib):
    import train_step
    assert list(train_step.lookahead([])) == []
    assert list(train_step.lookahead([7])) == [(7, None)]
    assert list(train_step.lookahead(iter("abc"))) == [("a", "b"), ("b", "c"), ("c", None)]


def test_eager_stepper_needs_inputs(built_lib):
    import train_step
    net = torch.nn.Linear(2, 2)
    st = train_step.CapturedStep(net, lambda ep, lab: ep, torch.zeros(1, 4, 3), graph=False, prefetch=None)
    assert st.launch == "eager" and st.graph is None
    with pytest.raises(ValueError, match="inputs"):
        st.step(None)


@pytest.mark.gpu
def test_replayed_captured_step_equals_the_eager_step():
    sys.path.insert(0, REPO)
    import bench
    import synth
    import train_step
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    dev = torch.device("cuda", 0)
    pcs = [synth.make_clouds(60 + i, 2, 20000, kind="room").to(dev) for i in range(4)]

    def criterion(ep, labels):
        return bench.loss_of(ep)

    watch = ("backbone.sa2.mlp_module.layer1.conv.weight", "decoder.0.linear1.weight", "vote_aggregation.mlp_module.layer0.conv.weight")

    def run(graph, announce):
        net = load_procedural(bench.build_model(0)).to(dev).train()
        zero_dropout(net)                      # the warm-up steps of a capture advance the dropout counters
        seen = {}

        def grab(mod, args, out):
            seen["ep"] = {k: v.detach().clone() for k, v in out.items() if k in ("sa1_inds", "sa2_inds", "seed_inds",
                          "seed_features", "last_center", "last_quad_center", "last_sem_cls_scores")}
        st = train_step.CapturedStep(net, criterion, {"point_clouds": pcs[0]}, graph=graph)
        hook = net.register_forward_hook(grab)
        params = dict(net.named_parameters())
        outs = []
        for pc, nxt in train_step.lookahead(pcs):
            loss = st.step({"point_clouds": pc}, None, next_inputs=({"point_clouds": nxt} if (nxt is not None and announce) else None))
            if graph:
                # the hook fired at capture time only: a replay rewrites the captured output tensors in place
                ep = {k: v.clone() for k, v in st.end_points.items() if k in ("sa1_inds", "sa2_inds", "seed_inds",
                      "seed_features", "last_center", "last_quad_center", "last_sem_cls_scores")}
            else:
                ep = seen["ep"]
            outs.append((loss.detach().clone(), ep, {n: params[n].grad.detach().float().clone() for n in watch}))
        hook.remove()
        torch.cuda.synchronize()
        assert st.launch == ("hipGraph replay" if graph else "eager")
        return outs

    def rel(x, y):
        return float((x.double() - y.double()).norm() / (y.double().norm() + 1e-30))

    want, again = run(False, True), run(False, True)
    # round 5: a step is bit-reproducible run to run -- forward (since round 4) AND backward (the CSR scatters accumulate in
    # f64, the LayerNorm / bias gradient reductions run in a fixed order; tools/repro_check.py: 0 of 519 gradients differ)
    for a, b in zip(want, again):
        # (the scalar is bench.py's stand-in loss: omnipq_sum_of_means folds its blocks with f32 atomics)
        assert abs(float(a[0]) - float(b[0])) <= 1e-6 * abs(float(a[0]))
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), k
        for n in watch:
            assert torch.equal(a[2][n], b[2][n]), n
    # A replay is NOT bit-equal to the eager launches: under capture the six layers' key sides are precomputed as pair launches on
    # a side stream (pq_transformer._OVERLAP_KEY_SIDE == "capture"), another -- equivalent -- order of the same f32 sums; the
    # e16 roundings of the backward pass amplify a last-bit difference to ~1e-2 on the backbone's weight gradients.
    noise, fwd_noise = 1e-2, 3e-7
    replays = {}
    for announce in (True, False):
        got = run(True, announce)
        replays[announce] = got
        for i, (a, b) in enumerate(zip(want, got)):
            # index outputs exact; float outputs and the loss to the forward pass's own run-to-run noise (the BatchNorm
            # statistics are folded with f64 atomics, whose order can move a last bit and with it a bf16 rounding)
            for k in a[1]:
                if a[1][k].is_floating_point():
                    assert rel(b[1][k], a[1][k]) <= 3 * fwd_noise + 1e-6, (announce, i, k, rel(b[1][k], a[1][k]), fwd_noise)
                else:
                    assert torch.equal(a[1][k], b[1][k]), (announce, i, k)
            assert abs(float(a[0]) - float(b[0])) <= 1e-5 * abs(float(a[0])), (announce, i, float(a[0]), float(b[0]))
            for n in watch:
                assert b[2][n].abs().sum() > 0, (announce, i, n)
                assert rel(b[2][n], a[2][n]) <= 3 * noise + 1e-4, (announce, i, n, rel(b[2][n], a[2][n]), noise)
    # ... but two CAPTURED steppers agree bit for bit, announced batches or not
    for a, b in zip(replays[True], replays[False]):
        assert abs(float(a[0]) - float(b[0])) <= 1e-6 * abs(float(a[0]))
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), k
        for n in watch:
            assert torch.equal(a[2][n], b[2][n]), n


@pytest.mark.gpu
def test_dead_cycles_are_collected_before_the_capture_begins_not_inside_it():
    """What died in a reference cycle before a CapturedStep is built -- an earlier stepper with its captured graph, say -- is
    collected before the capture begins: on ROCm the destructor of a captured graph synchronises the device, which a capture
    in progress refuses.  torch.cuda.graph itself does not collect.  The cycle here holds a plain object whose finalizer
    notes whether a capture was in progress; the automatic collector is off, so only the stepper's own collection finds it."""
    import gc
    import weakref
    sys.path.insert(0, REPO)
    import bench
    import synth
    import train_step
    dev = torch.device("cuda", 0)
    pc = synth.make_clouds(60, 2, 20000, kind="room").to(dev)
    net = bench.build_model(0).to(dev).train()

    class Node:
        pass

    seen = []
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        a, b = Node(), Node()
        a.other, b.other = b, a
        weakref.finalize(a, lambda: seen.append(torch.cuda.is_current_stream_capturing()))
        del a, b
        st = train_step.CapturedStep(net, lambda ep, labels: bench.loss_of(ep), {"point_clouds": pc})
    finally:
        if was_enabled:
            gc.enable()
    assert st.launch == "hipGraph replay"
    assert seen == [False]


@pytest.mark.gpu
def test_captured_step_trains_through_zero_grad_and_keeps_the_teacher_semantics():
    """(a) `optimizer.zero_grad()` (set_to_none=True, torch's default) before every replay must not orphan the
    graph's static gradient buffers -- the weights have to move; (b) the warm-up / capture runs on the example batch leave
    the BatchNorm running statistics and step counters of both networks untouched; (c) the teacher's weight averaging
    runs where the reference runs it (after optimizer.step(), train.py:560-576) with alpha = min(1 - 1/(step+1), decay)
    evaluated per call, and its forward's outputs reach the criterion."""
    sys.path.insert(0, REPO)
    import copy
    import bench
    import ema
    import synth
    import train_step
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    dev = torch.device("cuda", 0)
    pcs = [synth.make_clouds(80 + i, 2, 8192, kind="room").to(dev) for i in range(3)]
    net = load_procedural(bench.build_model(0)).to(dev).train()
    zero_dropout(net)
    teacher = copy.deepcopy(net)
    for p in teacher.parameters():
        p.requires_grad_(False)
    before = {k: v.detach().clone() for k, v in list(net.state_dict().items()) + [("t." + k, v) for k, v in teacher.state_dict().items()]}
    seen = []

    def criterion(ep, labels, teacher_ep):
        seen.append(teacher_ep)
        assert teacher_ep is not None and set(teacher_ep) == set(ep)
        return bench.loss_of(ep) + 0.1 * (ep["last_center"].float() - teacher_ep["last_center"].float()).square().mean()

    st = train_step.CapturedStep(net, criterion, {"point_clouds": pcs[0]}, teacher=teacher, ema=0.999,
                                 teacher_to_criterion=True)
    assert st.launch == "hipGraph replay" and seen
    after = dict(list(net.state_dict().items()) + [("t." + k, v) for k, v in teacher.state_dict().items()])
    for k, v in before.items():            # nothing moved: no optimizer yet, BatchNorm buffers restored, no EMA in the capture
        assert torch.equal(v, after[k]), k
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    w0 = net.decoder[0].linear1.weight.detach().clone()
    t0 = teacher.decoder[0].linear1.weight.detach().clone()
    for i, (pc, nxt) in enumerate(train_step.lookahead(pcs)):
        opt.zero_grad()                                            # set_to_none=True
        loss = st.step({"point_clouds": pc}, None, next_inputs=None if nxt is None else {"point_clouds": nxt})
        assert torch.isfinite(loss).item()
        assert all(p.grad is not None for p in net.decoder[0].parameters())
        opt.step()
        alpha = st.update_teacher(i)
        assert alpha == ema.ema_alpha(0.999, i) and (i > 0 or alpha == 0.0)
        if i == 0:                                                 # alpha = 0: the teacher IS the student after the first step
            assert torch.equal(teacher.decoder[0].linear1.weight, net.decoder[0].linear1.weight)
    torch.cuda.synchronize()
    assert not torch.equal(net.decoder[0].linear1.weight, w0), "the optimizer did not see the replay's gradients"
    assert not torch.equal(teacher.decoder[0].linear1.weight, t0)
    w1 = net.decoder[0].linear1.weight.detach().clone()
    t1 = teacher.decoder[0].linear1.weight.detach().clone()
    st.update_teacher(5)                                           # alpha = min(1 - 1/6, 0.999)
    a = 1.0 - 1.0 / 6.0
    want = t1 * a + (1.0 - a) * w1
    assert torch.allclose(teacher.decoder[0].linear1.weight, want, rtol=1e-6, atol=1e-8)


@pytest.mark.gpu
def test_whole_model_at_configs1_as_written_40k_points_batch_8_bf16_through_the_captured_step():
    """BASELINE configs[1] exactly as written -- 8 scenes x 40 000 points, bf16, forward + backward -- the shape the headline is
    measured on, through `CapturedStep` replays (until round 5 this shape ran only under bench.py, which
    asserts a finite loss and nothing else).  Properties that need no reference at this size: every float end_point and every
    parameter gradient of a REPLAYED step is finite and non-trivial; the backbone's index end_points equal the ORACLE's
    furthest-point sampling on the same clouds (two of the 8 scenes), seeds are the first 1024 sa1 picks, centres are the
    clouds' own points; and a replay gives the index keys of the same batch launched eagerly."""
    sys.path.insert(0, REPO)
    import bench
    import synth
    import train_step
    from oracle import oracle_ext
    dev = torch.device("cuda", 0)
    B, N = 8, 40000
    pcs = [synth.make_clouds(700 + i, B, N, kind="room") for i in range(3)]
    dpcs = [p.to(dev) for p in pcs]
    torch.manual_seed(3)
    net = bench.build_model(0).to(dev).train()

    def criterion(ep, labels):
        return bench.loss_of(ep)

    st = train_step.CapturedStep(net, criterion, {"point_clouds": dpcs[0]})
    assert st.launch == "hipGraph replay"
    int_keys = ("sa1_inds", "sa2_inds", "fp2_inds", "seed_inds")
    replayed = []
    for pc, nxt in train_step.lookahead(dpcs):
        loss = st.step({"point_clouds": pc}, None, next_inputs=None if nxt is None else {"point_clouds": nxt})
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        ep = st.end_points
        n_float = 0
        for k, v in ep.items():
            if torch.is_tensor(v) and v.is_floating_point():
                assert torch.isfinite(v).all().item(), k
                n_float += 1
        assert n_float >= 100 and len(ep) >= 119
        n_grad = 0
        for name, p in net.named_parameters():
            if p.grad is not None:
                assert torch.isfinite(p.grad).all().item(), name
                n_grad += 1
        assert n_grad >= 300
        for name in ("backbone.sa1.mlp_module.layer1.conv.weight", "backbone.sa2.mlp_module.layer0.conv.weight",
                     "vote_aggregation.mlp_module.layer0.conv.weight", "decoder.5.linear2.weight"):
            assert float(dict(net.named_parameters())[name].grad.abs().sum()) > 0, name
        replayed.append({k: ep[k].clone() for k in int_keys + ("sa1_xyz", "aggregated_vote_xyz")})
    assert st.replays == 3
    # index keys of the replays: int32, oracle-exact on scenes 0 and 7 of every batch
    for i, (pc, got) in enumerate(zip(pcs, replayed)):
        for k in int_keys:
            assert got[k].dtype == torch.int32, k
        assert tuple(got["sa1_inds"].shape) == (B, 2048) and tuple(got["sa2_inds"].shape) == (B, 1024)
        assert torch.equal(got["seed_inds"], got["sa1_inds"][:, :1024])
        for scene in (0, 7):
            cloud = pc[scene:scene + 1].contiguous()
            want1 = oracle_ext.furthest_point_sampling(cloud, 2048)
            assert torch.equal(got["sa1_inds"][scene:scene + 1].cpu(), want1), (i, scene)
            centres = cloud[0, want1[0].long()].unsqueeze(0).contiguous()
            assert torch.equal(got["sa1_xyz"][scene:scene + 1].cpu(), centres), (i, scene)
            want2 = oracle_ext.furthest_point_sampling(centres, 1024)
            assert torch.equal(got["sa2_inds"][scene:scene + 1].cpu(), want2), (i, scene)
    # the same batches launched eagerly by the same network (weights unchanged: no optimizer ran): same index keys
    eager = train_step.CapturedStep(net, criterion, {"point_clouds": dpcs[0]}, graph=False)
    for pc, got in zip(dpcs, replayed):
        seen = {}
        hook = net.register_forward_hook(lambda m, a, out: seen.update({k: out[k].detach().clone() for k in int_keys}))
        eager.step({"point_clouds": pc}, None)
        hook.remove()
        for k in int_keys:
            assert torch.equal(seen[k], got[k]), k
