"""CPU: the host logic of omni-pq_amd/device_data.py -- the epoch order of DeviceLoader (torch's DistributedSampler and
DataLoader batching, restated by comparison with the real ones), its length, and the refusals of SceneBank.add_scene.  Nothing
here touches a device: scenes are staged on the host until the first batch is assembled."""
import numpy as np
import pytest
import torch

import assemble_inputs as A


@pytest.fixture(autouse=True)
def _library(built_lib):
    """device_data binds the C-ABI library when it is imported"""
    yield


def bank_of(n_scenes, **kw):
    import device_data as D
    bank = D.SceneBank("cuda", A.Config, **kw)
    sc = A.scene("thin")
    for i in range(n_scenes):
        bank.add_scene(f"scene{i:04d}", sc["vertices"][:50], sc["normals"][:50], sc["instance_labels"][:50],
                       sc["semantic_labels"][:50], sc["boxes"], sc["rectangles"], sc["total_quad_num"], sc["horizontal_quads"])
    return D, bank


@pytest.mark.parametrize("n,world,batch,drop_last,shuffle", [(23, 1, 4, True, True), (23, 4, 2, True, True),
                                                             (23, 4, 2, False, True), (10, 3, 3, False, False),
                                                             (3, 8, 1, True, True)])
def test_epoch_order_is_the_distributed_samplers(n, world, batch, drop_last, shuffle):
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    D, bank = bank_of(n)
    data = list(range(n))
    shards = []
    for epoch in (0, 1, 5):
        seen = []
        for rank in range(world):
            loader = D.DeviceLoader(bank, batch, shuffle=shuffle, drop_last=drop_last, seed=7, rank=rank, world_size=world)
            loader.sampler.set_epoch(epoch)
            sampler = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=shuffle, seed=7)
            sampler.set_epoch(epoch)
            want = [b.tolist() for b in DataLoader(data, batch_size=batch, sampler=sampler, drop_last=drop_last)]
            assert loader.batches() == want, (epoch, rank)
            assert len(loader) == len(want) == len(DataLoader(data, batch_size=batch, sampler=sampler, drop_last=drop_last))
            assert loader.epoch_indices() == loader.epoch_indices(epoch) == list(sampler)          # a function of (seed, epoch)
            seen.append(loader.epoch_indices())
        # the rank::world shards partition the padded epoch
        total = -(-n // world) * world
        padded = [None] * total
        for rank, idx in enumerate(seen):
            padded[rank::world] = idx
        assert None not in padded and sorted(set(padded)) == data and len(padded) == total
        assert padded[n:] == (padded[:n] * world)[:total - n]
        shards.append(seen)
    if shuffle and n > 3:
        assert shards[0] != shards[1] and shards[1] != shards[2]                    # set_epoch changes the order
    other = D.DeviceLoader(bank, batch, shuffle=shuffle, seed=8, world_size=world)
    if shuffle and n > 3:
        other.sampler.set_epoch(0)
        assert other.epoch_indices() != shards[0][0]


def test_loader_arguments():
    D, bank = bank_of(4)
    for kw in ({"batch_size": 0}, {"batch_size": 2, "rank": 2, "world_size": 2}, {"batch_size": 2, "world_size": 0}):
        with pytest.raises(ValueError):
            D.DeviceLoader(bank, **kw)


def test_add_scene_refuses_what_the_item_cannot_hold():
    import device_data as D
    sc = A.scene("room")
    args = [sc["vertices"], sc["normals"], sc["instance_labels"], sc["semantic_labels"], sc["boxes"], sc["rectangles"],
            sc["total_quad_num"], sc["horizontal_quads"]]

    def refused(name, match, max_bytes=1 << 30, **change):
        bank = D.SceneBank("cuda", A.Config, max_bytes=max_bytes)
        a = list(args)
        for i, v in change.items():
            a[int(i[1:])] = v
        with pytest.raises(ValueError, match=name) as info:
            bank.add_scene(name, *a)
        assert match in str(info.value)
        assert len(bank) == 0 and bank.bytes == 0

    refused("many_boxes", "65 boxes", _4=np.tile(sc["boxes"][:1], (65, 1)))
    refused("many_rects", "33 rectangles", _5=np.tile(sc["rectangles"][:1], (33, 1)))
    refused("many_hquads", "5 horizontal", _7=np.zeros((5, 4, 3)))
    refused("many_instances", "1025 instances", _2=np.arange(3000) % 1025)
    refused("too_big", "max_bytes", max_bytes=10000)
    bad = sc["boxes"].copy()
    bad[3, 6] = 1                                            # a class outside nyu40ids
    refused("bad_class", "nyu40ids", _4=bad)
    bank = D.SceneBank("cuda", A.Config)
    assert bank.add_scene("ok", *args) == 0 and bank.add_scene("ok2", *args) == 1 and len(bank) == 2
    assert bank.pitch == 4 and bank.flavour == 0 and bank.bytes > 3000 * (16 + 12 + 12 + 8)
    with pytest.raises(ValueError, match="not both"):
        ark = A.scene("arkit")
        bank.add_unlabelled_scene("mixed", ark["vertices"], ark["normals"], ark["boxes"])
    unl = D.SceneBank("cuda")
    ark = A.scene("arkit")
    with pytest.raises(ValueError, match="crowded"):
        unl.add_unlabelled_scene("crowded", ark["vertices"], ark["normals"], np.tile(ark["boxes"][:1], (65, 1)))
    assert unl.add_unlabelled_scene("fine", ark["vertices"], ark["normals"], ark["boxes"]) == 0 and unl.pitch == 3
    # limits that are exactly met are accepted
    full = A.scene("full")
    assert D.SceneBank("cuda", A.Config).add_scene("full", full["vertices"], full["normals"], full["instance_labels"],
                                                  full["semantic_labels"], full["boxes"], full["rectangles"],
                                                  full["total_quad_num"], full["horizontal_quads"]) == 0


def test_static_parts_are_the_restatements():
    """what the bank computes once per scene equals the independent restatement bit for bit"""
    import assemble_restatement as R
    import device_data as D
    sc = A.scene("room")
    bank = D.SceneBank("cuda", A.Config)
    bank.add_scene("room", sc["vertices"], sc["normals"], sc["instance_labels"], sc["semantic_labels"], sc["boxes"],
                   sc["rectangles"], sc["total_quad_num"], sc["horizontal_quads"])
    pc, dense, n_inst = R.static_scannet(sc)
    host = bank._rows[0]
    assert host["points"].tobytes() == pc.tobytes() and np.array_equal(host["instance"], dense) and host["meta"][1] == n_inst
    assert host["meta"].tolist() == [3000, 40, 20, 7, 9, 2, 0, 0]
    ark = A.scene("arkit")
    unl = D.SceneBank("cuda")
    unl.add_unlabelled_scene("a", ark["vertices"], ark["normals"], ark["boxes"])
    got = unl._rows[0]["labels"][:64 * 7].reshape(64, 7)
    assert got[:10, :6].tobytes() == np.ascontiguousarray(R.static_arkit(ark)).tobytes() and not got[10:].any()
    packed = D.pack_params([(True, False, D.rotz(0.3), 1.1)])
    assert packed.shape == (1, 12) and packed[0, 0] == 1 and packed[0, 1] == 0 and packed[0, 11] == 1.1
    assert np.array_equal(packed[0, 2:11].reshape(3, 3), D.rotz(0.3))
    params = bank.draw_params(64)
    assert {p[0] for p in params} == {True, False} and all(0.85 <= p[3] < 1.15 for p in params)
    assert bank.draw_params(2, augment=False)[1] is D.IDENTITY
