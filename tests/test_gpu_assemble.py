"""Device-resident scenes on the HIP kernels (omni-pq_amd/device_data.py -> csrc/batch_assemble.hip, include/omnipq_data.h)
against (1) the outputs of the REFERENCE's `__getitem__` (tests/golden/assemble.npz) and (2) the numpy restatement
(tests/assemble_restatement.py), under the rules of tests/test_assemble_golden.py: integer keys exact; points, normals, votes
and ema_point_clouds bit-equal; box and quad floats within one float32 ulp.  Every batch mixes scenes of different row counts,
so the arena's offsets are exercised."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import assemble_inputs as A
import assemble_restatement as R
from test_assemble_golden import compare, gold, gold_item, params, restated

pytestmark = pytest.mark.gpu
DEV = "cuda"


def D():
    import device_data
    return device_data


def add(bank, name, sc, rows=None):
    rows = slice(None) if rows is None else slice(0, rows)
    return bank.add_scene(name, sc["vertices"][rows], sc["normals"][rows], sc["instance_labels"][rows],
                          sc["semantic_labels"][rows], sc["boxes"], sc["rectangles"], sc["total_quad_num"],
                          sc["horizontal_quads"])


def cut(sc, rows):
    return {k: (v[:rows] if k in ("vertices", "normals", "instance_labels", "semantic_labels") else v) for k, v in sc.items()}


_banks = {}


def labelled_bank():
    """room (3000 rows), thin (700), full (5000), and room cut to 1500 rows: four scenes, four offsets"""
    if "lab" not in _banks:
        bank = D().SceneBank(DEV, A.Config, seed=5)
        scenes = {"room": A.scene("room"), "thin": A.scene("thin"), "full": A.scene("full")}
        scenes["half"] = cut(scenes["room"], 1500)
        for name in ("room", "thin", "full", "half"):
            add(bank, name, scenes[name])
        _banks["lab"] = (bank, scenes)
    return _banks["lab"]


def unlabelled_bank():
    if "unl" not in _banks:
        bank = D().SceneBank(DEV, seed=6)
        ark = A.scene("arkit")
        scenes = {"small": cut(ark, 500), "arkit": ark, "mid": cut(ark, 2000)}
        for name in ("small", "arkit", "mid"):
            bank.add_unlabelled_scene(name, scenes[name]["vertices"], scenes[name]["normals"], scenes[name]["boxes"])
        _banks["unl"] = (bank, scenes)
    return _banks["unl"]


def item(batch, i):
    return {k: (v[i].cpu().numpy() if torch.is_tensor(v) else v[i]) for k, v in batch.items()}


def snapshot(bank):
    return {k: v.clone() for k, v in bank.upload().items() if torch.is_tensor(v)}


def unchanged(bank, before):
    for k, v in bank.upload().items():
        if torch.is_tensor(v):
            assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), f"the bank's {k} was modified"


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def other_params(i):
    return (i % 2 == 0, i % 3 == 0, D().rotz(0.07 * (i + 1) + (i % 4) * np.pi / 2), 0.9 + 0.05 * i)


def same_batch(a, b):
    for k, v in a.items():
        if torch.is_tensor(v):
            if not torch.equal(v.contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)):
                return False
    return True


@pytest.mark.parametrize("k,order", [(1024, ("half", "room", "thin", "room")), (2048, ("thin", "full", "room"))])
def test_labelled_batch_equals_restatement_and_fixture(k, order):
    """supplied choices and parameters: the fixture's for the cases of this k (room, thin, plain = room with identity
    parameters; full), seeded ones for the scenes that fill the batch"""
    bank, scenes = labelled_bank()
    before = snapshot(bank)
    cases = {1024: [None, "room", "thin", "plain"], 2048: [None, "full", None]}[k]
    rs = np.random.RandomState(k)
    ch, ema, prm = [], [], []
    for i, (scene, case) in enumerate(zip(order, cases)):
        n = scenes[scene]["vertices"].shape[0]
        if case is None:
            ch.append(rs.choice(n, k, replace=n < k))
            ema.append(rs.choice(n, k, replace=n < k))
            prm.append(other_params(i))
        else:
            ch.append(gold(case, "choices"))
            ema.append(gold(case, "ema_choices"))
            prm.append(params(case))
    slots = [bank.names.index(s) for s in order]
    batch = bank.assemble(slots, prm, dev_i32(np.stack(ch)), dev_i32(np.stack(ema)), num_points=k)
    assert batch["scan_name"] == list(order) and batch["use_gt"].dtype == torch.bool and batch["use_gt"].all()
    assert batch["point_clouds"].shape == (len(order), k, 4) and batch["vote_label_mask"].dtype == torch.int64
    for i, (scene, case) in enumerate(zip(order, cases)):
        got = item(batch, i)
        if case is None:
            want = R.scannet_item(scenes[scene], A.Config, ch[i].astype(np.int32), ema[i].astype(np.int32), prm[i], slot=slots[i])
            compare(got, want, (k, i, scene, "restatement"))
        else:
            want = dict(restated(case))
            want["scan_idx"] = np.array(slots[i]).astype(np.int64)           # the slot in THIS bank
            compare(got, want, (k, i, case, "restatement"))
            seen = compare(got, gold_item(case), (k, i, case, "fixture"), skip=("scan_idx",))
            assert len(seen) == 28 and "use_gt" in seen
        assert np.array_equal(got["choices"], ch[i]) and np.array_equal(got["ema_choices"], ema[i])
    unchanged(bank, before)


def test_unlabelled_batch_equals_restatement_and_fixture():
    bank, scenes = unlabelled_bank()
    before = snapshot(bank)
    k, order = 1024, ("small", "arkit", "mid")
    rs = np.random.RandomState(3)
    ch = [rs.choice(500, k), gold("arkit", "choices"), rs.choice(2000, k, replace=False)]
    ema = [rs.choice(500, k), gold("arkit", "ema_choices"), rs.choice(2000, k, replace=False)]
    prm = [other_params(0), params("arkit"), other_params(2)]
    batch = bank.assemble([0, 1, 2], prm, dev_i32(np.stack(ch)), dev_i32(np.stack(ema)), num_points=k)
    assert "vote_label" not in batch and "semantic_labels" not in batch and batch["point_clouds"].shape == (3, k, 3)
    for i, scene in enumerate(order):
        got = item(batch, i)
        want = R.arkit_item(scenes[scene], ch[i].astype(np.int32), ema[i].astype(np.int32), prm[i])
        compare(got, want, (i, scene, "restatement"))
    seen = compare(item(batch, 1), gold_item("arkit"), "fixture")
    assert len(seen) == 12 and int(batch["flip_x_axis"][1]) == 0                 # both flips drawn: the flag is cleared
    assert batch["flip_x_axis"].tolist() == [0, 0, 1] and not batch["flip_y_axis"].any()      # (x, y), (x, y), (x) alone
    unchanged(bank, before)


def test_device_draw_is_the_restatements_hash():
    bank, scenes = labelled_bank()
    order, k = ("room", "thin", "full", "half"), 1024
    slots = [bank.names.index(s) for s in order]
    prm = [other_params(i) for i in range(4)]
    bank.seed.fill_(1234)
    first = bank.assemble(slots, prm, num_points=k)
    for i, scene in enumerate(order):
        n = scenes[scene]["vertices"].shape[0]
        got = item(first, i)
        for key, stream_id in (("choices", 0), ("ema_choices", 1)):
            assert np.array_equal(got[key], R.draw(1234, stream_id, i, n, k)), (scene, key)
            assert got[key].min() >= 0 and got[key].max() < n
            if n >= k:
                assert len(set(got[key].tolist())) == k, (scene, key, "not distinct")
        assert not np.array_equal(got["choices"], got["ema_choices"])
        compare(got, R.scannet_item(scenes[scene], A.Config, got["choices"], got["ema_choices"], prm[i], slot=slots[i]),
                (scene, "restatement on the drawn rows"))
    first = {k_: (v.clone() if torch.is_tensor(v) else v) for k_, v in first.items()}
    again = bank.assemble(slots, prm, num_points=k)
    assert same_batch(first, again)                                              # the same seed word: the same batch
    bank.seed.add_(1)
    other = bank.assemble(slots, prm, num_points=k)
    assert not torch.equal(other["choices"], first["choices"]) and not torch.equal(other["ema_choices"], first["ema_choices"])
    assert np.array_equal(other["choices"][2].cpu().numpy(), R.draw(1235, 0, 2, 5000, k))
    # a negative seed word is the same 64 bits read as unsigned
    bank.seed.fill_(-2)
    neg = bank.assemble(slots[:1], prm[:1], num_points=k)
    assert np.array_equal(neg["choices"][0].cpu().numpy(), R.draw((1 << 64) - 2, 0, 0, 3000, k))


def test_inclusion_is_uniform():
    """n = 1000, k = 400, 256 seed values: every row's inclusion count is Binomial(256, 0.4); all within 6 sigma of 102.4
    (sigma = 7.84; false-alarm probability about 2e-6 over the 1000 rows)"""
    sc = cut(A.scene("room"), 1000)
    bank = D().SceneBank(DEV, A.Config)
    add(bank, "thousand", sc)
    buf = bank.make_buffers(1, 400)
    counts = torch.zeros(1000, dtype=torch.int64, device=DEV)
    one = torch.ones(400, dtype=torch.int64, device=DEV)
    for seed in range(256):
        bank.seed.fill_(seed)
        batch = bank.assemble([0], [D().IDENTITY], num_points=400, out=buf)
        counts.index_add_(0, batch["choices"][0].long(), one)
        if seed in (0, 100, 255):
            assert np.array_equal(batch["choices"][0].cpu().numpy(), R.draw(seed, 0, 0, 1000, 400))
    counts = counts.cpu().numpy()
    sigma = (256 * 0.4 * 0.6) ** 0.5
    assert counts.sum() == 256 * 400
    assert np.abs(counts - 102.4).max() <= 6 * sigma, (counts.min(), counts.max())


def test_supplied_indices_outside_the_scene_give_zero_rows():
    bank, scenes = labelled_bank()
    k = 1024
    order = ("thin", "room")
    slots = [bank.names.index(s) for s in order]
    ch = np.stack([gold("thin", "choices"), gold("room", "choices")]).copy()
    ema = np.stack([gold("thin", "ema_choices"), gold("room", "ema_choices")]).copy()
    ch[0, 5], ch[0, 6], ch[1, 0], ch[1, k - 1] = -1, 700, 3000, -1            # n of thin is 700, of room 3000
    ema[1, 17], ema[0, 3] = 3000, -5
    prm = [params("thin"), params("room")]
    batch = bank.assemble(slots, prm, dev_i32(ch), dev_i32(ema), num_points=k)
    for i, scene in enumerate(order):
        got = item(batch, i)
        want = R.scannet_item(scenes[scene], A.Config, ch[i], ema[i], prm[i], slot=slots[i])
        compare(got, want, (scene, "restatement"))                           # the neighbouring rows stay exact
    for i, p in ((0, 5), (0, 6), (1, 0), (1, k - 1)):
        for key in ("point_clouds", "vertex_normals", "vote_label", "pcl_color", "semantic_labels", "vote_label_mask"):
            assert not batch[key][i, p].any(), (key, i, p)
        assert int(batch["point_instance_label"][i, p]) == -1
    assert not batch["ema_point_clouds"][1, 17].any() and not batch["ema_point_clouds"][0, 3].any()
    assert batch["ema_point_clouds"][1, 16].any() and batch["point_clouds"][0, 4].any()


def test_colour_columns_ride_along():
    """use_color: seven columns (:116-122) -- xyz augmented, the normalised colours copied, the height scaled; no pcl_color"""
    sc = A.scene("thin")
    bank = D().SceneBank(DEV, A.Config, use_color=True)
    add(bank, "thin", sc)
    k = 256
    rs = np.random.RandomState(9)
    ch, ema = rs.choice(700, k, replace=False), rs.choice(700, k, replace=False)
    prm = other_params(1)
    batch = bank.assemble([0], [prm], dev_i32(ch[None]), dev_i32(ema[None]), num_points=k)
    pc = sc["vertices"][:, 0:6].copy()
    pc[:, 3:] = (pc[:, 3:] - D().MEAN_COLOR_RGB) / 256.0
    pc = np.concatenate([pc, np.expand_dims(pc[:, 2] - np.percentile(pc[:, 2], 0.99), 1)], 1)
    assert pc.dtype == np.float32 and bank.pitch == 7 and "pcl_color" not in batch
    want = R._points(pc[ch], np.ones(k, bool), *prm, 6)
    assert batch["point_clouds"][0].cpu().numpy().tobytes() == want.tobytes()
    assert batch["ema_point_clouds"][0].cpu().numpy().tobytes() == pc[ema].tobytes()
    assert (want[:, 3:6] == pc[ch][:, 3:6]).all() and not (want[:, 6] == pc[ch][:, 6]).all()


def test_identity_parameters_copy_the_rows():
    """augment=False: the reference does no arithmetic, so a -0.0 coordinate stays -0.0 (x * 1 + y * 0 would make it +0.0);
    and a caller-owned buffer of another dtype is refused instead of being written as raw bytes"""
    sc = cut(A.scene("thin"), 300)
    sc["vertices"] = sc["vertices"].copy()
    sc["normals"] = sc["normals"].copy()
    sc["vertices"][0, 0] = sc["vertices"][1, 1] = sc["normals"][2, 0] = -0.0
    bank = D().SceneBank(DEV, A.Config)
    add(bank, "zeros", sc)
    k = 128
    ch = np.arange(k, dtype=np.int32)
    batch = bank.assemble([0], None, dev_i32(ch[None]), dev_i32(ch[None]), num_points=k, augment=False)
    got = item(batch, 0)
    compare(got, R.scannet_item(sc, A.Config, ch, ch, R.IDENTITY), "identity")
    assert np.signbit(got["point_clouds"][0, 0]) and np.signbit(got["point_clouds"][1, 1]) and np.signbit(got["vertex_normals"][2, 0])
    assert got["point_clouds"][:, :4].tobytes() == got["ema_point_clouds"].tobytes()
    buf = bank.make_buffers(1, k)
    buf["vote_label_mask"] = buf["vote_label_mask"].to(torch.int32)
    with pytest.raises(ValueError, match="vote_label_mask"):
        bank.assemble([0], None, num_points=k, augment=False, out=buf)
    del buf["rot_mat"]
    with pytest.raises(ValueError, match="rot_mat"):
        bank.assemble([0], None, num_points=k, augment=False, out=buf)


def test_static_buffers_replay_from_a_graph():
    """out= buffers, device-resident slots and parameters: the four launches captured in one torch.cuda.graph (a single
    stream, nothing on the side), replayed twice with the seed word advanced in between == two eager calls with the same
    two seed values, bit for bit"""
    bank, scenes = labelled_bank()
    k = 1024
    slots = dev_i32([0, 1, 2, 3])
    prm = torch.from_numpy(D().pack_params([other_params(i) for i in range(4)])).to(DEV)
    eager = []
    for seed in (100, 101):
        bank.seed.fill_(seed)
        got = bank.assemble(slots, prm, num_points=k)
        assert "scan_name" not in got
        eager.append({k_: v.clone() for k_, v in got.items()})
    assert not same_batch(eager[0], eager[1])
    buf = bank.make_buffers(4, k)
    bank.seed.fill_(7)
    bank.assemble(slots, prm, num_points=k, out=buf)                             # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = bank.assemble(slots, prm, num_points=k, out=buf)
    for key, v in static.items():
        assert v.data_ptr() == buf[key].data_ptr()
    for seed, want in zip((100, 101), eager):
        bank.seed.fill_(seed)
        graph.replay()
        torch.cuda.synchronize()
        assert same_batch(want, static), seed
    assert np.array_equal(static["choices"][1].cpu().numpy(), R.draw(101, 0, 1, 700, k))


def test_labels_go_through_get_loss_like_the_fixtures():
    """a labelled `room` batch through models/loss_helper_pq.py:get_loss with seeded predictions (tests/loss_inputs.py): the
    loss on the device's labels equals the loss on the fixture's labels bit for bit -- dtypes and shapes are the consumer's"""
    import loss_helper_pq
    import loss_inputs
    from test_get_loss_oracle import build
    bank, scenes = labelled_bank()
    k, B = 1024, 2
    slot = bank.names.index("room")
    ch = dev_i32(np.stack([gold("room", "choices")] * B))
    ema = dev_i32(np.stack([gold("room", "ema_choices")] * B))
    batch = bank.assemble([slot] * B, [params("room")] * B, ch, ema, num_points=k)
    fixture = gold_item("room")
    lab, pred = loss_inputs.make(21, B=B, K=256, KQ=256, num_seed=256, N=k)
    keep = {key: lab[key] for key in ("seed_inds", "seed_xyz", "aggregated_vote_xyz", "aggregated_sample_xyz")}
    losses = []
    for source in ("device", "fixture"):
        ep, _ = build(keep, pred, device=DEV)
        for key in fixture:
            if key in ("scan_name", "use_gt", "pcl_color"):
                continue
            ep[key] = batch[key] if source == "device" else torch.from_numpy(np.stack([fixture[key]] * B)).to(DEV)
        loss, ep = loss_helper_pq.get_loss(ep, loss_inputs.Config, pc_loss=True)
        assert torch.isfinite(loss).item()
        losses.append(loss.detach().clone())
    assert losses[0].dtype == losses[1].dtype and torch.equal(losses[0].view(torch.int32), losses[1].view(torch.int32)), losses


def test_device_loader_yields_resident_batches():
    bank, _ = labelled_bank()
    loader = D().DeviceLoader(bank, batch_size=2, seed=3, num_points=512, side_stream=True)
    loader.sampler.set_epoch(2)
    want = loader.batches()
    got = list(loader)
    assert len(got) == len(loader) == 2
    for batch, slots in zip(got, want):
        assert batch["scan_idx"].tolist() == slots and batch["scan_name"] == [bank.names[s] for s in slots]
        pc = batch["point_clouds"]
        assert pc.is_cuda and pc.cuda(non_blocking=True) is pc and pc.shape == (2, 512, 4)
        assert torch.isfinite(pc).all() and batch["vote_label_mask"].max() <= 1
    assert not torch.equal(got[0]["choices"], got[1]["choices"])
    plain = list(D().DeviceLoader(bank, batch_size=2, seed=3, num_points=512, shuffle=False))       # on the caller's stream
    assert [b["scan_idx"].tolist() for b in plain] == [[0, 1], [2, 3]]


@pytest.mark.parametrize("side_stream", [False, True])
def test_loader_announces_the_batch_the_consumer_runs_next(side_stream):
    """net=: the backbone keeps ONE sampling plan, keyed on the tensor (Pointnet2Backbone._key).  Whenever a batch is handed
    out the plan in flight must be that batch's -- with a stub that keeps one plan the way the backbone does, and with the
    real network, whose forward() must find its plan and never sample a cloud a second time."""
    bank, _ = labelled_bank()

    class OnePlan:
        def __init__(self):
            self.plan, self.calls = None, 0

        @staticmethod
        def key(t):
            return (t.data_ptr(), t._version, tuple(t.shape))

        def prefetch(self, inputs):
            self.plan, self.calls = self.key(inputs["point_clouds"]), self.calls + 1

    stub = OnePlan()
    loader = D().DeviceLoader(bank, batch_size=1, seed=3, num_points=512, net=stub, side_stream=side_stream)
    handed = 0
    for batch in loader:
        handed += 1
        assert stub.plan == stub.key(batch["point_clouds"]) and stub.calls == handed
    assert handed == 4

    from pq_transformer import PQ_Transformer
    torch.manual_seed(0)
    net = PQ_Transformer(input_feature_dim=1, num_class=18, num_proposal=256, num_quad_proposal=256, num_heading_bin=1,
                         num_size_cluster=18, mean_size_arr=A.Config.mean_size_arr).to(DEV)
    net.train()
    backbone = net.backbone
    launched = []
    real = backbone._launch_plan

    def counting(pointcloud, *args, **kw):
        launched.append(backbone._key(pointcloud))
        return real(pointcloud, *args, **kw)

    backbone._launch_plan = counting
    loader = D().DeviceLoader(bank, batch_size=2, seed=3, num_points=4096, net=net, side_stream=side_stream)
    ran = []
    for batch in loader:
        ran.append(backbone._key(batch["point_clouds"]))
        ep = net({"point_clouds": batch["point_clouds"]})
        assert ep["sa1_inds"].shape[0] == 2 and torch.isfinite(ep["last_center"].float()).all()
    torch.cuda.synchronize()
    assert len(ran) == 2 and launched == ran, (launched, ran)          # one sampling per batch, started by the loader
