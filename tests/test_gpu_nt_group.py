"""GPU: group launches (include/omnipq_sa.h: omnipq_pair_group).  n independent small launches of one kind -- the plain and
the BatchNorm-backward data-gradient GEMMs on the K-resident small-tile path, omnipq_bn_bwd_apply_fused -- held back and sent
out as ONE grid give the bits of the same calls issued one after the other: every workgroup of the group kernels runs the
program of the single launch on its own problem.  The f64 column sums are compared bit for bit too: a problem here has at
most four row tiles, so a column's total is the sum of at most four f32 partials, which f64 adds exactly in any order."""
import ctypes

import pytest
import torch

import capi

pytestmark = pytest.mark.gpu

ROWS, KS, NS = (40, 64, 200), (64, 288), (32, 128, 288)
LL, D = ctypes.c_longlong, ctypes.c_double


def dev():
    return torch.device("cuda:0")


def _lib():
    lib = capi.lib()
    lib.omnipq_pair_flush.restype = ctypes.c_longlong
    lib.omnipq_pair_hold.restype = None
    return lib


def _gemm_problem(gen, i, kind):
    """problem i of a group: the shapes cycle through ROWS x KS x NS at different rates, so a group mixes them"""
    M, K, N = ROWS[i % 3], KS[(i // 2) % 2], NS[(i + i // 3) % 3]
    p = dict(kind=kind, M=M, N=N, K=K,
             A=torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev()),
             B=torch.randn((N, K), generator=gen).to(torch.bfloat16).to(dev()))
    if kind == "plain":
        p["bias"] = torch.randn(N, generator=gen).to(dev())
    else:
        p["Y"] = torch.randn((M, N), generator=gen).to(torch.bfloat16).to(dev())
        for name in ("a", "b", "mean"):
            p[name] = torch.randn(N, generator=gen).to(dev())
        p["invstd"] = (torch.rand(N, generator=gen) + 0.5).to(dev())
    return p


def _gemm(p):
    """issue the problem's GEMM -> (C, sums | None)"""
    M, N, K = p["M"], p["N"], p["K"]
    C = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    if p["kind"] == "plain":
        capi.ok("omnipq_gemm_nt_e16_bias", M, N, K, capi.P(p["A"]), K, capi.P(p["B"]), K, capi.P(C), N, capi.P(p["bias"]))
        return C, None
    sums = torch.zeros((2, N), device=dev(), dtype=torch.float64)
    capi.ok("omnipq_gemm_nt_e16_bnbwd", M, N, K, capi.P(p["A"]), K, capi.P(p["B"]), K, capi.P(C), N, capi.P(p["Y"]),
            capi.P(p["a"]), capi.P(p["b"]), capi.P(p["mean"]), capi.P(p["invstd"]), capi.P(sums), ctypes.c_void_p(0))
    return C, sums


def _apply_problem(gen, i):
    P, C = (40, 200)[i % 2], (32, 288)[(i // 2) % 2]
    p = dict(P=P, C=C, dX=torch.randn((P, C), generator=gen).to(torch.bfloat16).to(dev()),
             Y=torch.randn((P, C), generator=gen).to(torch.bfloat16).to(dev()),
             sums=torch.randn((2, C), generator=gen, dtype=torch.float64).to(dev()))
    for name in ("a", "b", "mean"):
        p[name] = torch.randn(C, generator=gen).to(dev())
    p["invstd"] = (torch.rand(C, generator=gen) + 0.5).to(dev())
    return p


def _apply(p):
    """-> (dY, dbeta_dgamma)"""
    P, C = p["P"], p["C"]
    dY = torch.full((P, C), float("nan"), device=dev(), dtype=torch.bfloat16)
    dbg = torch.full((2, C), float("nan"), device=dev())
    capi.ok("omnipq_bn_bwd_apply_fused", LL(P), C, D(float(P)), capi.P(p["dX"]), capi.P(p["Y"]), capi.P(p["a"]), capi.P(p["b"]),
            capi.P(p["mean"]), capi.P(p["invstd"]), capi.P(p["sums"]), capi.P(dY), capi.P(dbg))
    return dY, dbg


def _same(got, want):
    for g, w in zip(got, want):
        for tg, tw in zip(g, w):
            assert (tg is None) == (tw is None)
            if tg is not None:
                assert torch.equal(tg, tw)         # (NaN never equals itself: an element nobody wrote fails here)


def _grouped(lib, problems, issue):
    """the problems as one group -> (results, shared grids launched)"""
    n = len(problems)
    before = int(lib.omnipq_pair_flush())
    assert lib.omnipq_pair_group(n) == 0
    got = []
    for i, p in enumerate(problems):
        if i < n - 1:
            lib.omnipq_pair_hold()
        got.append(issue(p))
        assert lib.omnipq_pair_held() == (i + 1 if i < n - 1 else 0)
    grids = int(lib.omnipq_pair_flush()) - before
    assert lib.omnipq_pair_held() == 0
    return got, grids


@pytest.mark.parametrize("n", [1, 2, 3, 7, 14])
@pytest.mark.parametrize("kind", ["plain", "bnbwd", "apply"])
def test_group_equals_the_same_calls_unheld(kind, n):
    lib = _lib()
    gen = torch.Generator().manual_seed(100 * n + len(kind))
    if kind == "apply":
        problems, issue = [_apply_problem(gen, i) for i in range(n)], _apply
    else:
        problems, issue = [_gemm_problem(gen, i, kind) for i in range(n)], _gemm
    want = [issue(p) for p in problems]
    got, grids = _grouped(lib, problems, issue)
    assert grids == (1 if n > 1 else 0)              # one grid for the group (a group of one is a plain launch)
    torch.cuda.synchronize()
    _same(got, want)


def test_a_stranger_sends_the_held_ones_out_singly_and_in_order():
    """three plain GEMMs held, then a GEMM of another kind: no shared grid, every result as unheld -- and in issue order: the
    three held ones write the SAME output buffer, and what it holds in the end is the third one's."""
    lib = _lib()
    gen = torch.Generator().manual_seed(5)
    M, N, K = 200, 128, 64
    A = [torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev()) for _ in range(3)]
    B = torch.randn((N, K), generator=gen).to(torch.bfloat16).to(dev())
    bias = torch.randn(N, generator=gen).to(dev())
    stranger = _gemm_problem(gen, 2, "bnbwd")
    C = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)

    def plain(a, out):
        capi.ok("omnipq_gemm_nt_e16_bias", M, N, K, capi.P(a), K, capi.P(B), K, capi.P(out), N, capi.P(bias))

    want = torch.empty_like(C)
    plain(A[2], want)
    want_stranger = _gemm(stranger)
    before = int(lib.omnipq_pair_flush())
    assert lib.omnipq_pair_group(5) == 0
    for i in range(3):
        lib.omnipq_pair_hold()
        plain(A[i], C)
        assert lib.omnipq_pair_held() == i + 1
    lib.omnipq_pair_hold()
    got_stranger = _gemm(stranger)
    assert lib.omnipq_pair_held() == 0                # the stranger sent them out and went out itself
    assert int(lib.omnipq_pair_flush()) == before
    torch.cuda.synchronize()
    assert torch.equal(C, want)
    _same([got_stranger], [want_stranger])


def test_a_group_that_ends_short_goes_out_on_flush_and_the_pair_protocol_is_unchanged():
    lib = _lib()
    gen = torch.Generator().manual_seed(6)
    problems = [_gemm_problem(gen, i, "plain") for i in range(3)]
    want = [_gemm(p) for p in problems]
    before = int(lib.omnipq_pair_flush())
    assert lib.omnipq_pair_group(7) == 0
    got = []
    for p in problems:
        lib.omnipq_pair_hold()
        got.append(_gemm(p))
    assert lib.omnipq_pair_held() == 3
    assert int(lib.omnipq_pair_flush()) == before and lib.omnipq_pair_held() == 0      # singly
    _same(got, want)
    assert lib.omnipq_pair_group(0) != 0 and lib.omnipq_pair_group(15) != 0             # sizes the protocol does not take
    # no group open: hold one, pair with the next; a third launch goes out alone
    lib.omnipq_pair_hold()
    got = [_gemm(problems[0])]
    assert lib.omnipq_pair_held() == 1
    got.append(_gemm(problems[1]))
    assert lib.omnipq_pair_held() == 0
    got.append(_gemm(problems[2]))
    assert lib.omnipq_pair_held() == 0
    assert int(lib.omnipq_pair_flush()) == before + 1
    torch.cuda.synchronize()
    _same(got, want)
