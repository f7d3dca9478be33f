"""GPU: the sa1 sampling level split over two steps (Pointnet2Backbone.prefetch_head / prefetch(resume=True),
train_step.CapturedStep(lookahead=2)) changes WHEN indices are computed and nothing else: index outputs equal, and float
outputs, loss and gradients held to what tests/test_train_step.py establishes between two captured steppers (torch.equal on
outputs and gradients, 1e-6 relative on the stand-in loss)."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu

INDEX_KEYS = ("sa1_inds", "sa2_inds", "seed_inds", "fp2_inds")
OUT_KEYS = ("sa1_inds", "sa2_inds", "seed_inds", "seed_features", "last_center", "last_quad_center", "last_sem_cls_scores")
WATCH = ("backbone.sa2.mlp_module.layer1.conv.weight", "decoder.0.linear1.weight",
         "vote_aggregation.mlp_module.layer0.conv.weight")


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("k", [1, 1433, 2047])
def test_head_then_resumed_chain_gives_the_plain_forwards_indices(k):
    import synth
    import pointnet2_utils
    from procedural import load_procedural
    from test_oracle_golden import build_model
    net = load_procedural(build_model(0)).to(dev()).eval()
    pc = synth.make_clouds(90, 2, 20000, kind="room").to(dev())
    with torch.no_grad():
        net.backbone.forget_plan()
        want = net({"point_clouds": pc})
        before = net.backbone.resumed_levels
        net.prefetch_head({"point_clouds": pc}, k)
        assert net.backbone._head is not None and net.backbone._head.rounds == k
        net.prefetch({"point_clouds": pc}, resume=True)
        assert net.backbone.resumed_levels == before + 1          # the chain did continue the head
        assert net.backbone._head is None and net.backbone._tail is None and net.backbone._plan is not None
        got = net({"point_clouds": pc})
        assert net.backbone._plan is None                          # ... and forward() took that chain
        # the head of ANOTHER cloud is not continued
        other = synth.make_clouds(91, 2, 20000, kind="room").to(dev())
        net.prefetch_head({"point_clouds": other}, k)
        net.prefetch({"point_clouds": pc}, resume=True)
        assert net.backbone.resumed_levels == before + 1
        again = net({"point_clouds": pc})
    torch.cuda.synchronize()
    for key in INDEX_KEYS:
        assert torch.equal(got[key], want[key]), key
        assert torch.equal(again[key], want[key]), key
    for key in ("sa1_xyz", "sa4_xyz", "seed_features"):
        assert torch.equal(got[key], want[key]), key
    pointnet2_utils._ext.fps_check()
    net.backbone.forget_plan()
    assert net.backbone._head is None and net.backbone._tail is None


def run_stepper(pcs, lookahead, announce, with_teacher):
    """-> per step (loss, outputs, watched gradients, teacher's index outputs); announce: how many batches ahead (0, 1, 2)"""
    import bench
    import train_step
    import pointnet2_utils
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    net = load_procedural(bench.build_model(0)).to(dev()).train()
    zero_dropout(net)
    teacher = None
    if with_teacher:
        teacher = copy.deepcopy(net)
        for p in teacher.parameters():
            p.requires_grad_(False)

        def criterion(ep, labels, teacher_ep):
            return bench.loss_of(ep) + 0.1 * (ep["last_center"].float() - teacher_ep["last_center"].float()).square().mean()
    else:
        def criterion(ep, labels):
            return bench.loss_of(ep)
    st = train_step.CapturedStep(net, criterion, {"point_clouds": pcs[0]}, teacher=teacher, teacher_to_criterion=with_teacher,
                                 lookahead=lookahead)
    assert st.launch == "hipGraph replay"
    eager_heads = []
    if lookahead == 2:
        real = st._sample_head_now
        st._sample_head_now = lambda: (eager_heads.append(st.replays), real())[1]
        assert st.nxt2 is not None and st.head_rounds == 1024 and st.footprint == "small"
        assert (st.nxt2_t is not None) == with_teacher
    params = dict(net.named_parameters())
    batches = [{"point_clouds": p} for p in pcs]
    outs = []
    for i, batch in enumerate(batches):
        kw = {}
        if announce >= 1 and i + 1 < len(batches):
            kw["next_inputs"] = batches[i + 1]
        if announce >= 2 and i + 2 < len(batches):
            kw["after_next_inputs"] = batches[i + 2]
        loss = st.step(batch, None, **kw)
        ep = {k: v.clone() for k, v in st.end_points.items() if k in OUT_KEYS}
        tep = {k: st.teacher_end_points[k].clone() for k in INDEX_KEYS} if with_teacher else {}
        outs.append((loss.detach().clone(), ep, {n: params[n].grad.detach().float().clone() for n in WATCH}, tep))
    torch.cuda.synchronize()
    assert st.launch == "hipGraph replay" and st.replays == len(pcs)
    pointnet2_utils._ext.fps_check()
    if lookahead == 2:
        # a head is sampled in front of a replay exactly when the batch that becomes `next` was not announced two calls ahead
        want_eager = {2: [0], 1: list(range(len(pcs) - 1)), 0: []}[announce]
        assert eager_heads == want_eager, (announce, eager_heads)
        assert net.backbone._head_side is not None
    return outs


@pytest.mark.parametrize("with_teacher", [False, True])
def test_split_step_equals_todays_step_however_far_ahead_batches_are_announced(with_teacher):
    import synth
    pcs = [synth.make_clouds(60 + i, 2, 20000, kind="room").to(dev()) for i in range(5)]
    base = run_stepper(pcs, 1, 1, with_teacher)
    for name, announce in (("lookahead=2, fully announced", 2), ("lookahead=2, next only", 1), ("lookahead=2, nothing", 0)):
        got = run_stepper(pcs, 2, announce, with_teacher)
        for i, (a, b) in enumerate(zip(base, got)):
            for k in a[1]:
                if not a[1][k].is_floating_point():
                    assert torch.equal(a[1][k], b[1][k]), (name, i, k)
            for k in a[3]:
                assert torch.equal(a[3][k], b[3][k]), (name, i, "teacher", k)
        for i, (a, b) in enumerate(zip(base, got)):
            print(f"{name} step {i}: loss {float(a[0])!r} vs {float(b[0])!r}; float outputs equal: "
                  f"{[k for k in a[1] if torch.equal(a[1][k], b[1][k])]}; gradients equal: "
                  f"{[n for n in WATCH if torch.equal(a[2][n], b[2][n])]}")
            assert abs(float(a[0]) - float(b[0])) <= 1e-6 * abs(float(a[0])), (name, i, float(a[0]), float(b[0]))
            for k in a[1]:
                assert torch.equal(a[1][k], b[1][k]), (name, i, k)
            for n in WATCH:
                assert b[2][n].abs().sum() > 0, (name, i, n)
                assert torch.equal(a[2][n], b[2][n]), (name, i, n)


def test_lookahead_1_allocates_nothing_of_the_split_and_rejects_after_next_inputs():
    import bench
    import synth
    import train_step
    from procedural import load_procedural
    pcs = [synth.make_clouds(60 + i, 2, 20000, kind="room").to(dev()) for i in range(3)]
    net = load_procedural(bench.build_model(0)).to(dev()).train()
    st = train_step.CapturedStep(net, lambda ep, labels: bench.loss_of(ep), {"point_clouds": pcs[0]})
    assert st.lookahead == 1 and st.head_rounds is None and st.nxt2 is None and st.nxt2_t is None
    st.step({"point_clouds": pcs[0]}, None, next_inputs={"point_clouds": pcs[1]})
    bb = net.backbone
    assert bb._head_side is None and bb._head is None and bb._tail is None and bb.resumed_levels == 0
    assert not any(isinstance(k, tuple) and k and k[0] == "split" for k in bb.__dict__.get("_plan_bufs", {}))
    with pytest.raises(ValueError, match="lookahead=2"):
        st.step({"point_clouds": pcs[1]}, None, next_inputs={"point_clouds": pcs[2]}, after_next_inputs={"point_clouds": pcs[2]})
    with pytest.raises(ValueError):
        train_step.CapturedStep(net, lambda ep, labels: bench.loss_of(ep), {"point_clouds": pcs[0]}, lookahead=3, graph=False)
    with pytest.raises(ValueError):
        train_step.CapturedStep(net, lambda ep, labels: bench.loss_of(ep), {"point_clouds": pcs[0]}, lookahead=2,
                                head_rounds=2048, graph=False)
    torch.cuda.synchronize()


def test_sampling_streams_are_never_the_capture_stream_nor_each_other():
    """torch hands streams out of a pool of 32 per device round-robin, so a new Stream object can be the stream graphs are
    captured on; the plan of the first captured batch is launched before the capture and waited for inside it, which the
    runtime refuses when the sampling stream itself is capturing.  The backbone's streams skip such a draw."""
    import backbone_module
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(8, device=dev())
    with torch.cuda.graph(graph):                      # makes sure torch has picked its capture stream
        x.add_(1)
    cap = torch.cuda.graph.default_capture_stream.cuda_stream
    handles = set()
    for _ in range(70):                                # more than two turns of the pool
        bb = backbone_module.Pointnet2Backbone()
        side = bb._side_stream(dev())
        head = bb._head_stream(dev())
        assert side.cuda_stream != cap and head.cuda_stream != cap and side.cuda_stream != head.cuda_stream
        assert bb._side_stream(dev()) is side and bb._head_stream(dev()) is head
        handles.update((side.cuda_stream, head.cuda_stream))
    assert len(handles) >= 8                           # (it is still the pool's streams that are used)
