"""GPU: inference.CapturedInference at the model's smallest configuration (the constructor arguments of
test_gpu_rows_infer.py::test_model_eval_forward_..., 2 x 4096 points): the replayed graph gives, bit for bit, the records of a
second runner built with graph=False on the same weights and of detect_* applied to a plain eager forward -- for announced
batches, for an unannounced one and with prefetch=None -- and the runner refuses a net in train mode and a mutated config.
The network, the batches and the plain-forward reference are made once per module and never changed."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)

pytestmark = pytest.mark.gpu
MEANS = (np.arange(54, dtype=np.float32).reshape(18, 3) % 5 + 0.5)
PREFIXES = ("last_", "proposal_")


class DatasetConfig:
    num_class = 18
    num_heading_bin = 1
    num_size_cluster = 18
    mean_size_arr = MEANS.astype(np.float64)

    def class2angle(self, pred_cls, residual, to_label_format=True):
        return 0


def config():
    return {"remove_empty_box": True, "use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True,
            "per_class_proposal": True, "conf_thresh": 0.05, "dataset_config": DatasetConfig()}


def snapshot(dets):
    return {p: tuple(None if d is None else d.record.clone() for d in pair) for p, pair in dets.items()}


def same(a, b):
    assert sorted(a) == sorted(b)
    for p in a:
        for x, y, kind in zip(a[p], b[p], ("boxes", "quads")):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.equal(x, y), (p, kind, int((x != y).sum()))


@pytest.fixture(scope="module")
def world():
    import ap_helper_pq
    import synth
    from pq_transformer import PQ_Transformer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = PQ_Transformer(input_feature_dim=1, num_class=18, num_proposal=256, num_quad_proposal=256, num_heading_bin=1,
                         num_size_cluster=18, mean_size_arr=MEANS).to(dev).eval()
    batches = []
    for seed in (81, 82, 83, 84, 85):
        cloud = synth.make_clouds(seed, 2, 4096, kind="room").to(dev)
        batches.append(torch.cat([cloud[..., :3], cloud[..., 2:3]], dim=2).contiguous())
    cfg = config()
    plain = []
    for batch in batches:                                    # detect_* on a plain eager forward, no runner
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            ep = net({"point_clouds": batch})
        ep["point_clouds"] = batch
        plain.append({p: (ap_helper_pq.detect_predictions(ep, cfg, p).record.clone(),
                          ap_helper_pq.detect_quad_predictions(ep, cfg, p).record.clone()) for p in PREFIXES})
    torch.cuda.synchronize()
    return net, batches, cfg, plain


def test_replay_reproduces_the_eager_runner_and_the_plain_forward_bit_for_bit(world):
    import inference
    net, (b0, b1, b2, b3, b4), cfg, plain = world
    runner = inference.CapturedInference(net, b4, cfg, prefixes=PREFIXES)
    assert runner.launch == "hipGraph replay" and runner.graph is not None and runner.replays == 0
    got = [snapshot(runner.run(b0, next_inputs=b1)),         # b0 was never announced: sampled in front of its replay
           snapshot(runner.run(b1, next_inputs=b2)),         # announced
           snapshot(runner.run(None, next_inputs=None)),     # announced, taken as is (b2)
           snapshot(runner.run(b3))]                         # nothing was announced
    held = runner.end_points["last_center"]
    got.append(snapshot(runner.run(b1, next_inputs=b2)))
    got.append(snapshot(runner.run(b0)))                     # b2 was announced, b0 arrives: copied in and sampled up front
    assert runner.replays == 6 and runner.end_points["last_center"] is held          # static outputs
    order = (0, 1, 2, 3, 1, 0)
    for g, i in zip(got, order):
        same(g, plain[i])
    assert not torch.equal(plain[0]["last_"][0], plain[1]["last_"][0])                # the batches do differ
    # what the last run left on the host is what parse_* would return
    boxes, quads = runner.run(b3)["last_"]
    pred_map, pred_mask = boxes.to_lists()
    assert pred_mask.shape == (2, 256) and pred_mask.any() and sum(len(x) for x in pred_map) > 0
    q_map, q_mask, q_corners = quads.to_lists()
    assert q_mask.any() and [len(x) for x in q_map] == [int(n) for n in quads.count.cpu()]
    assert torch.equal(boxes.record, plain[3]["last_"][0])

    # a forward of the same network between two runs takes the sampling chain's buffers: forget_next() says so
    runner.run(b1, next_inputs=b2)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        net({"point_clouds": b3})
    runner.forget_next()
    same(snapshot(runner.run(b2)), plain[2])

    eager = inference.CapturedInference(net, b4, cfg, prefixes=PREFIXES, graph=False)
    assert eager.launch == "eager" and eager.graph is None
    for (cur, nxt), i in zip(((b0, b1), (b1, b2), (b2, None), (b3, None)), (0, 1, 2, 3)):
        same(snapshot(eager.run(cur, next_inputs=nxt)), plain[i])


def test_prefetch_none_gives_the_same_records(world):
    import inference
    net, (b0, b1, b2, b3, b4), cfg, plain = world
    runner = inference.CapturedInference(net, b4, cfg, prefixes=PREFIXES, prefetch=None)
    assert runner.launch == "hipGraph replay"
    for batch, i in ((b2, 2), (b0, 0), (b3, 3)):
        same(snapshot(runner.run(batch)), plain[i])
    only_quads = inference.CapturedInference(net, b4, cfg, objects=False, graph=False)
    dets = only_quads.run(b1)
    assert sorted(dets) == ["last_"] and dets["last_"][0] is None
    assert torch.equal(dets["last_"][1].record, plain[1]["last_"][1])


def test_a_net_in_train_mode_and_a_mutated_config_are_refused(world):
    import inference
    net, (b0, b1, b2, b3, b4), cfg, plain = world
    net.train()
    try:
        with pytest.raises(RuntimeError, match=r"net\.eval\(\)"):
            inference.CapturedInference(net, b4, cfg, graph=False)
    finally:
        net.eval()
    cfg = dict(cfg)
    runner = inference.CapturedInference(net, b4, cfg, graph=False)
    same(snapshot(runner.run(b0)), {"last_": plain[0]["last_"]})
    cfg["conf_thresh"] = 0.5
    with pytest.raises(RuntimeError, match="new runner"):
        runner.run(b0)
    cfg["conf_thresh"] = 0.05
    cfg["dataset_config"].mean_size_arr = cfg["dataset_config"].mean_size_arr + 1.0          # an instance attribute now
    try:
        with pytest.raises(RuntimeError, match="new runner"):
            runner.run(b0)
    finally:
        del cfg["dataset_config"].mean_size_arr
    same(snapshot(runner.run(b0)), {"last_": plain[0]["last_"]})
    net.train()
    try:
        with pytest.raises(RuntimeError, match=r"net\.eval\(\)"):
            runner.run(b0)
    finally:
        net.eval()
    with pytest.raises(ValueError, match="nothing to detect"):
        inference.CapturedInference(net, b4, cfg, objects=False, quads=False, graph=False)
