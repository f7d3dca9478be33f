"""GPU: omnipq_furthest_point_sampling_resume through the raw C ABI against the CPU oracle.

The oracle cannot resume and does not need to: FPS is prefix-stable, so its m = k run IS the state after the rounds [0, k)
(indices 0 .. k-1 and the running minimum distances with the picks 0 .. k-2 folded in).  Everything here is exact equality
-- indices and `temp` bit for bit (BASELINE.json north_star: index operators are bit-exact); no tolerance is involved.
No test feeds a corrupt state: the kernel's clamp of idxs[:, first-1] is verified by reading the code.
"""
import ctypes
import functools

import pytest
import torch

import capi
from oracle import oracle_ext
from test_gpu_parity import FPS_CASES, cloud

pytestmark = pytest.mark.gpu
SENTINEL = -7
SMALL = 1          # OMNIPQ_FPS_SMALL_FOOTPRINT


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def oracle_state(xyz, m):
    """-> (idx (b, m) i32, temp (b, n) f32) of the oracle's sampling of m points"""
    b, n, _ = xyz.shape
    idx = torch.zeros((b, m), dtype=torch.int32)
    tmp = torch.full((b, n), 1e10)
    oracle_ext.lib().oracle_furthest_point_sampling(b, n, m, ctypes.c_void_p(xyz.data_ptr()), ctypes.c_void_p(tmp.data_ptr()),
                                                    ctypes.c_void_p(idx.data_ptr()))
    return idx, tmp


@functools.lru_cache(maxsize=None)
def case_cloud(kind, b, n):
    return cloud(kind, 5, b, n)


def fresh(xyz, m):
    b, n, _ = xyz.shape
    return (torch.full((b, m), SENTINEL, device=xyz.device, dtype=torch.int32),
            torch.full((b, n), 1e10, device=xyz.device, dtype=torch.float32))


def resume(xyz, idx, tmp, first, count, flags=0):
    b, n, _ = xyz.shape
    capi.ok("omnipq_furthest_point_sampling_resume", b, n, idx.shape[1], first, count, capi.P(xyz), capi.P(tmp), capi.P(idx),
            ctypes.c_uint(flags))


def check_clean():
    rc = capi.lib().omnipq_fps_check(capi.stream())
    assert rc == 0, capi.lib().omnipq_error_string(rc).decode()


def split_points(m):
    return sorted({k for k in (1, 2, m // 3, 1023, 1024, 1025, m - 1) if 1 <= k <= m - 1})


def assert_state(idx, tmp, want_idx, want_tmp, upto, what):
    got = idx.cpu()
    assert torch.equal(got[:, :upto], want_idx[:, :upto]), \
        f"{what}: first mismatch at {(got[:, :upto] != want_idx[:, :upto]).nonzero()[:3].tolist()}"
    assert bool((got[:, upto:] == SENTINEL).all()), f"{what}: wrote past column {upto}"
    assert torch.equal(tmp.cpu(), want_tmp), f"{what}: temp differs in {int((tmp.cpu() != want_tmp).sum())} places"


@pytest.mark.parametrize("kind,b,n,m", FPS_CASES)
def test_resume_in_two_and_three_pieces_equals_the_oracle(kind, b, n, m):
    xyz = case_cloud(kind, b, n)
    gx = xyz.to(dev())
    want_idx, want_tmp = oracle_state(xyz, m)
    # the whole sampling as one piece
    idx, tmp = fresh(gx, m)
    resume(gx, idx, tmp, 0, m)
    assert_state(idx, tmp, want_idx, want_tmp, m, "[0, m)")
    check_clean()
    for k in split_points(m):
        head_idx, head_tmp = oracle_state(xyz, k)
        assert torch.equal(head_idx, want_idx[:, :k])                 # prefix stability, on the oracle itself
        idx, tmp = fresh(gx, m)
        resume(gx, idx, tmp, 0, k)
        assert_state(idx, tmp, head_idx, head_tmp, k, f"[0, {k})")
        resume(gx, idx, tmp, k, m - k)
        assert_state(idx, tmp, want_idx, want_tmp, m, f"[{k}, {m})")
        check_clean()
    if m >= 3:
        a, c = m // 3, m - m // 4 - 1
        assert 1 <= a < c < m
        idx, tmp = fresh(gx, m)
        resume(gx, idx, tmp, 0, a)
        resume(gx, idx, tmp, a, c - a)
        mid_idx, mid_tmp = oracle_state(xyz, c)
        assert_state(idx, tmp, mid_idx, mid_tmp, c, f"[0, {a}) + [{a}, {c})")
        resume(gx, idx, tmp, c, m - c)
        assert_state(idx, tmp, want_idx, want_tmp, m, f"three pieces {a}, {c}")
        check_clean()


@pytest.mark.parametrize("kind,b,n,m", [c for c in FPS_CASES if c[2] > 8192])
@pytest.mark.parametrize("head_flags,tail_flags", [(0, SMALL), (SMALL, 0)])
def test_pieces_may_use_different_launch_shapes(kind, b, n, m, head_flags, tail_flags):
    """The state between two pieces is (temp, idx[:, :first]) and nothing else: the head with the default footprint and the
    tail with 16 points per thread on fewer workgroups, and the reverse."""
    xyz = case_cloud(kind, b, n)
    gx = xyz.to(dev())
    want_idx, want_tmp = oracle_state(xyz, m)
    k = m // 2
    idx, tmp = fresh(gx, m)
    resume(gx, idx, tmp, 0, k, head_flags)
    head_idx, head_tmp = oracle_state(xyz, k)
    assert_state(idx, tmp, head_idx, head_tmp, k, f"[0, {k}) flags {head_flags}")
    resume(gx, idx, tmp, k, m - k, tail_flags)
    assert_state(idx, tmp, want_idx, want_tmp, m, f"[{k}, {m}) flags {tail_flags}")
    check_clean()


def degenerate_clouds():
    yield "inside the skip ball", torch.rand(2, 500, 3, generator=torch.Generator().manual_seed(1)) * 0.01, 40
    yield "all duplicates", torch.ones(2, 1500, 3), 20
    g = torch.arange(12, dtype=torch.float32)
    lat = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3) + 1.0
    for n in (1728, 1000, 600):
        yield f"lattice {n}", lat[:, :n].contiguous(), 200


def test_ties_and_degenerate_inputs_through_a_split_in_the_middle():
    for name, xyz, m in degenerate_clouds():
        gx = xyz.to(dev())
        want_idx, want_tmp = oracle_state(xyz, m)
        k = m // 2
        idx, tmp = fresh(gx, m)
        resume(gx, idx, tmp, 0, k)
        head_idx, head_tmp = oracle_state(xyz, k)
        assert_state(idx, tmp, head_idx, head_tmp, k, f"{name}: head")
        resume(gx, idx, tmp, k, m - k)
        assert_state(idx, tmp, want_idx, want_tmp, m, f"{name}: tail")
        if name == "inside the skip ball":
            assert int(idx.abs().sum()) == 0          # nothing selectable: every round falls back to index 0
        check_clean()


@pytest.mark.parametrize("kind,b,n,m", FPS_CASES)
def test_ex_and_resume_of_everything_are_the_same_call(kind, b, n, m):
    gx = case_cloud(kind, b, n).to(dev())
    for flags in (0, SMALL):
        want, want_tmp = capi.fps(gx, m, flags=flags)
        idx, tmp = fresh(gx, m)
        resume(gx, idx, tmp, 0, m, flags)
        assert torch.equal(idx, want) and torch.equal(tmp, want_tmp)
    plain, plain_tmp = capi.fps(gx, m)
    assert torch.equal(plain, want) and torch.equal(plain_tmp, want_tmp)
    check_clean()


def test_an_empty_piece_writes_nothing():
    gx = case_cloud("room", 2, 20000).to(dev())
    idx, tmp = fresh(gx, 64)
    tmp.fill_(3.0)
    resume(gx, idx, tmp, 5, 0)
    resume(gx, idx, tmp, 64, 0)
    assert bool((idx == SENTINEL).all()) and bool((tmp == 3.0).all())
    check_clean()


@pytest.mark.parametrize("kind,b,n,m", [("room", 2, 40000, 2048), ("room", 2, 4096, 512), ("room", 2, 1024, 256)])
def test_head_and_tail_on_two_streams_ordered_by_an_event(kind, b, n, m):
    """The exchange workspace is per stream; the sampling's state is not: a tail on another stream, ordered behind the head
    by an event, continues it."""
    xyz = case_cloud(kind, b, n)
    gx = xyz.to(dev())
    want_idx, want_tmp = oracle_state(xyz, m)
    k = (2 * m) // 3
    idx, tmp = fresh(gx, m)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    done = torch.cuda.Event()
    with torch.cuda.stream(s1):
        resume(gx, idx, tmp, 0, k)
        done.record(s1)
    s2.wait_event(done)
    with torch.cuda.stream(s2):
        resume(gx, idx, tmp, k, m - k, SMALL)
    torch.cuda.current_stream().wait_stream(s2)
    torch.cuda.synchronize()
    assert_state(idx, tmp, want_idx, want_tmp, m, "two streams")
    check_clean()
