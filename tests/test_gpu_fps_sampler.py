"""GPU: pointnet2_utils.FurthestPointSampler -- a sampling advanced in pieces, captured into a graph, handed from one sampler
to another -- against furthest_point_sample and the CPU oracle.  Exact equality throughout."""
import pytest
import torch

import synth
from oracle import oracle_ext

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("b,n,m,pieces,small", [(2, 40000, 2048, (1, 700, 323, 1, 1000), False),
                                                (2, 40000, 2048, (1433,), True),
                                                (3, 4096, 512, (100, 0, 411), False),
                                                (2, 1024, 256, (255,), False),
                                                (2, 200, 64, (5, 5, 5), False)])
def test_sampler_in_uneven_pieces_equals_furthest_point_sample(b, n, m, pieces, small):
    import pointnet2_utils
    xyz = synth.make_clouds(41, b, n, kind="room")[..., :3].contiguous().to(dev())
    want = pointnet2_utils.furthest_point_sample(xyz, m)
    s = pointnet2_utils.FurthestPointSampler(xyz.shape, m, xyz.device, small_footprint=small)
    assert s.position == 0 and not s.done
    with pytest.raises(RuntimeError):
        s.advance()
    s.begin(xyz)
    pos = 0
    for r in pieces:
        pos += r
        assert s.advance(r) == pos == s.position and not s.done
        assert torch.equal(s.idx[:, :pos], want[:, :pos])
    assert s.advance() == m and s.done
    assert s.advance(10) == m                      # nothing left: a no-op
    assert torch.equal(s.idx, want)
    assert torch.equal(want.cpu(), oracle_ext.furthest_point_sampling(xyz.cpu(), m))
    # growing a sample: the first m picks of a longer sampling are the m-sampling
    big = pointnet2_utils.FurthestPointSampler((b, n), m + 100, xyz.device).begin(xyz)
    big.advance(m)
    assert torch.equal(big.idx[:, :m], want)
    big.advance()
    assert torch.equal(big.idx, pointnet2_utils.furthest_point_sample(xyz, m + 100))
    # begin() starts over on the same buffers
    other = synth.make_clouds(42, b, n, kind="room")[..., :3].contiguous().to(dev())
    s.begin(other)
    assert s.position == 0
    s.advance(m // 2)
    s.advance()
    assert torch.equal(s.idx, pointnet2_utils.furthest_point_sample(other, m))
    with pytest.raises(ValueError):
        s.begin(other[:, :-1].contiguous())
    pointnet2_utils._ext.fps_check()


@pytest.mark.parametrize("b,n,m,k", [(2, 20000, 600, 250), (2, 2048, 512, 100)])
def test_captured_begin_and_advance_replay_on_new_cloud_contents(b, n, m, k):
    import pointnet2_utils
    clouds = [synth.make_clouds(50 + i, b, n, kind="room")[..., :3].contiguous() for i in range(3)]
    static = clouds[0].to(dev())
    s = pointnet2_utils.FurthestPointSampler(static.shape, m, static.device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        s.begin(static)                            # warm-up on the capture's stream: its exchange workspace exists afterwards
        s.advance(k)
        s.advance()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        s.begin(static)
        s.advance(k)
        s.advance()
    assert s.done
    for xyz in clouds[1:] + clouds[:1]:
        static.copy_(xyz)
        s.idx.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s.idx.cpu(), oracle_ext.furthest_point_sampling(xyz, m))
    pointnet2_utils._ext.fps_check()


def test_copy_state_from_continues_where_the_original_stands():
    import pointnet2_utils
    b, n, m, k = 2, 40000, 1024, 700
    xyz = synth.make_clouds(43, b, n, kind="room")[..., :3].contiguous().to(dev())
    a = pointnet2_utils.FurthestPointSampler(xyz.shape, m, xyz.device).begin(xyz)
    a.advance(k)
    c = pointnet2_utils.FurthestPointSampler(xyz.shape, m, xyz.device, small_footprint=True)
    c.idx.fill_(-3)
    c.copy_state_from(a)
    assert c.position == k and not c.done
    assert bool((c.idx[:, k:] == -3).all())        # only idx[:, :position] travels
    c.advance()
    a.advance()
    assert a.done and c.done
    assert torch.equal(c.idx, a.idx) and torch.equal(c.temp, a.temp)
    assert torch.equal(a.idx, pointnet2_utils.furthest_point_sample(xyz, m))
    with pytest.raises(ValueError):
        pointnet2_utils.FurthestPointSampler((b, n), m + 1, xyz.device).copy_state_from(a)
    pointnet2_utils._ext.fps_check()
