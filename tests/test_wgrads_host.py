"""CPU: sa_fused.deferred_wgrads end to end -- the cases of the placement rules (tests/wgrads_cases.py) collected with add /
add_sa on CPU operands, the grouped launch replaced by its statement in include/omnipq_sa.h on host memory, uncleared memory
poisoned with NaN."""
import math

import pytest
import torch

import wgrads_cases


@pytest.mark.parametrize("name", wgrads_cases.NAMES)
def test_deferred_wgrads_on_host_memory(name, built_lib, monkeypatch):
    """After the block every parameter's `.grad` is dY^T X (bf16 operands of 37 rows, widths 8-32), cropped and rotated as the
    item says, the bias gradient the column sums; to 1e-6 relative, element by element: the stand-in computes in float64, so
    only the float32 stores round (the operands are positive, no sum cancels; an element nothing collected is exactly 0).  A
    `.grad` that existed before the block has the result added to it; nothing is assigned before the block ends."""
    import sa_fused
    case = wgrads_cases.cases()[name]
    launches = []

    def launch(fn, anchor, *args):
        assert all(p.grad is before[id(p)] for p in case.params), "a .grad was replaced before the block ended"
        launches.append(fn.__name__)
        wgrads_cases.grouped_tn_on_host(fn, anchor, *args)

    monkeypatch.setattr(sa_fused, "_call", launch)
    monkeypatch.setattr(sa_fused, "empty_f32", lambda shape, device: torch.full(tuple(shape), math.nan))
    monkeypatch.setattr(sa_fused, "zeros_f32", lambda n, device: torch.zeros(n))
    gen = torch.Generator().manual_seed(5)
    for i, p in enumerate(case.params):
        p.grad = torch.rand(p.shape, generator=gen) + 0.5 if i % 2 == 0 else None
    before = {id(p): p.grad for p in case.params}
    start = {id(p): None if p.grad is None else p.grad.clone() for p in case.params}
    with sa_fused.deferred_wgrads() as dfr:
        for it in case.items:
            if case.sa:
                dfr.add_sa(it.dY, it.X, it.M, it.N, it.P, it.wt, it.crop)
            else:
                dfr.add(it.dY, it.X, it.M, it.N, it.P, it.wt, it.crop, it.bt)
        assert len(dfr.sa_items if case.sa else dfr.items) == len(case.items) and dfr._assign == [] and launches == []
        assert all(p.grad is before[id(p)] for p in case.params)
    assert launches == ["omnipq_gemm_tn_grouped"] and sa_fused.deferred_wgrads.active is None
    want = wgrads_cases.collected(case.items)
    assert set(want) == {id(p) for p in case.params}
    for p in case.params:
        expect = want[id(p)][1].view(p.shape) + (0 if start[id(p)] is None else start[id(p)].double())
        assert p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        if start[id(p)] is not None:
            assert p.grad is before[id(p)], "an existing .grad is added to, not replaced"
        assert torch.allclose(p.grad.double(), expect, rtol=1e-6, atol=0.0), (name, (p.grad.double() - expect).abs().max())
