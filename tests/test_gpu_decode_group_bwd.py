"""GPU: omnipq_decode_pair_group_bwd (include/omnipq_decoder.h) -- the decode backward of several stages, four per launch --
against one omnipq_decode_pair_bwd call per stage in the same order: both heads' dy, the quad head's base gradients and the
common sink of the object head's base gradients, bit for bit.  The sink is a sequential f32 sum over the stages; the group
kernel forms it in one thread per element in the single calls' order, so the comparison is exact."""
import ctypes

import pytest
import torch

import capi

pytestmark = pytest.mark.gpu

B, K, KQ, NH, NS, NCLS = 2, 5, 3, 1, 18, 18
WIDTH = 5 + 2 * NH + 4 * NS + NCLS
LD, LDQ = 128, 32
N2 = [1, 1, 1, 1, 1, 1, 3, 3, 1, 1]


def dev():
    return torch.device("cuda:0")


def _grad(gen, shape, how):
    """how: 0 bf16 | 1 f32 | 2 None | 3 an expanded scalar (every stride 0: what SumOfMeans.backward hands out), f32 |
    4 the same in bf16"""
    if how == 2:
        return None
    dtype = torch.bfloat16 if how in (0, 4) else torch.float32
    if how >= 3:
        return torch.randn([1] * len(shape), generator=gen).to(dtype).to(dev()).expand(*shape)
    return torch.randn(shape, generator=gen).to(dtype).to(dev())


def _descriptors(gs):
    ptrs, strides, flags = [], [], []
    for g in gs:
        if g is None:
            ptrs.append(None)
            strides += [0, 0, 0, 0]
            flags.append(0)
            continue
        st = list(g.stride())
        ptrs.append(g.data_ptr())
        strides += st if len(st) == 4 else st + [0]
        flags.append(int(g.dtype == torch.bfloat16))
    return ptrs, strides, flags


def _stage(gen, s):
    hs = [(B, K, 2), (B, K, 3), (B, K, NH), (B, K, NH), (B, K, NH), (B, K, NS), (B, K, NS, 3), (B, K, NS, 3), (B, K, 3),
          (B, K, NCLS)]
    qs = [(B, KQ, 2), (B, KQ, 3), (B, KQ, 3), (B, KQ, 2)]
    # the kinds rotate with the stage and the output, so that every output meets every kind (the object centre's gradient,
    # which feeds the sink, is None in stages 0 and 5 and an expanded scalar in stages 1, 2 and 6)
    gh = [_grad(gen, sh, (s + 2 * i) % 5) for i, sh in enumerate(hs)]
    gq = [_grad(gen, sh, (2 * s + i + 1) % 5) for i, sh in enumerate(qs)]
    yh = torch.randn((B * K, LD), generator=gen).to(torch.bfloat16).to(dev())
    yq = torch.randn((B * KQ, LDQ), generator=gen).to(torch.bfloat16).to(dev())
    return dict(yh=yh, yq=yq, gh=gh, gq=gq, means=(torch.rand((NS, 3), generator=gen) + 0.2).to(dev()),
                norm=(torch.rand(1, generator=gen) + 1.0).to(dev()))


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _outputs(n, own_dbh):
    nan = float("nan")
    return dict(dyh=[torch.full((B * K, LD), nan, device=dev(), dtype=torch.bfloat16) for _ in range(n)],
                dyq=[torch.full((B * KQ, LDQ), nan, device=dev(), dtype=torch.bfloat16) for _ in range(n)],
                dbq=[torch.full((B, KQ, 3), nan, device=dev()) for _ in range(n)],
                dbh=[torch.full((B, K, 3), nan, device=dev()) for _ in range(n)] if own_dbh else None)


def _single_calls(stages, sink, start):
    out = _outputs(len(stages), sink is None)
    scale = float(torch.tensor(torch.pi / NH, dtype=torch.float32))
    for s, st in enumerate(stages):
        ph, sh, fh = _descriptors(st["gh"])
        pq, sq, fq = _descriptors(st["gq"])
        dbh = sink if sink is not None else out["dbh"][s]
        acc = int(sink is not None and (start or s > 0))
        capi.ok("omnipq_decode_pair_bwd", B * K, K, NH, NS, NCLS, capi.P(st["yh"]), LD, capi.P(st["means"]),
                ctypes.c_float(scale), _arr(ctypes.c_void_p, ph), _arr(ctypes.c_int, sh), _arr(ctypes.c_int, N2),
                _arr(ctypes.c_int, fh), capi.P(out["dyh"][s]), LD, capi.P(dbh), B * KQ, KQ, capi.P(st["yq"]), LDQ,
                capi.P(st["norm"]), _arr(ctypes.c_void_p, pq), _arr(ctypes.c_int, sq), _arr(ctypes.c_int, fq),
                capi.P(out["dyq"][s]), LDQ, capi.P(out["dbq"][s]), acc)
    return out


def _group_call(stages, sink, start):
    n = len(stages)
    out = _outputs(n, sink is None)
    scale = float(torch.tensor(torch.pi / NH, dtype=torch.float32))
    ph, sh, fh, pq, sq, fq = [], [], [], [], [], []
    for st in stages:
        for dst, part in zip((ph, sh, fh), _descriptors(st["gh"])):
            dst += part
        for dst, part in zip((pq, sq, fq), _descriptors(st["gq"])):
            dst += part

    def ptrs(ts):
        return _arr(ctypes.c_void_p, [t.data_ptr() for t in ts])

    capi.ok("omnipq_decode_pair_group_bwd", n, B * K, K, NH, NS, NCLS, ptrs([st["yh"] for st in stages]), LD,
            ptrs([st["means"] for st in stages]), ctypes.c_float(scale), _arr(ctypes.c_void_p, ph), _arr(ctypes.c_int, sh),
            _arr(ctypes.c_int, N2), _arr(ctypes.c_int, fh), ptrs(out["dyh"]), LD,
            ptrs(out["dbh"]) if sink is None else ctypes.c_void_p(0), B * KQ, KQ, ptrs([st["yq"] for st in stages]), LDQ,
            ptrs([st["norm"] for st in stages]), _arr(ctypes.c_void_p, pq), _arr(ctypes.c_int, sq), _arr(ctypes.c_int, fq),
            ptrs(out["dyq"]), LDQ, ptrs(out["dbq"]), capi.P(sink), int(start))
    return out


@pytest.fixture(scope="module")
def seven_stages():
    gen = torch.Generator().manual_seed(11)
    return [_stage(gen, s) for s in range(7)]


@pytest.mark.parametrize("with_sink,start", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("n", [1, 2, 4, 5, 7])
def test_group_decode_backward_equals_one_call_per_stage(seven_stages, n, with_sink, start):
    """start: the sink already holds a sum (a call that continues an earlier one)"""
    stages = seven_stages[:n]
    gen = torch.Generator().manual_seed(n)
    first = torch.randn((B, K, 3), generator=gen).to(dev()) if start else torch.full((B, K, 3), float("nan"), device=dev())
    sink_want = first.clone() if with_sink else None
    sink_got = first.clone() if with_sink else None
    want = _single_calls(stages, sink_want, start)
    got = _group_call(stages, sink_got, start)
    torch.cuda.synchronize()
    for key in ("dyh", "dyq", "dbq") + (() if with_sink else ("dbh",)):
        for s in range(n):
            assert torch.equal(got[key][s], want[key][s]), (key, s)
    if with_sink:
        assert torch.equal(sink_got, sink_want)


def test_group_decode_backward_refuses_what_it_cannot_run():
    lib = capi.lib()
    p = ctypes.c_void_p(0x1000)                       # never dereferenced: refused first
    null = ctypes.c_void_p(0)
    one = (ctypes.c_void_p * 1)(0x1000)
    n2 = (ctypes.c_int * 10)(*N2)

    def call(nstage, ldyh=LD, dbaseh=null, sink=null):
        return lib.omnipq_decode_pair_group_bwd(nstage, B * K, K, NH, NS, NCLS, one, ldyh, one, ctypes.c_float(1.0), p, p, n2, p,
                                                one, LD, dbaseh, B * KQ, KQ, one, LDQ, one, p, p, p, one, LDQ, null, sink, 0,
                                                null)

    assert call(0) == 10001 and call(1, ldyh=WIDTH - 1) == 10001
    assert call(1, dbaseh=one, sink=p) == 10001       # a sink and a stage's own buffer
