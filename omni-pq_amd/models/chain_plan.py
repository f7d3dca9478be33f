"""The prefetched sampling chain of Pointnet2Backbone (backbone_module.py), as data: where every piece of the chain's flat
int32 buffer lies (`chain_layout`, a pure function of integers), the typed views of such a buffer (`chain_views`, the only
place that slices it) and the host records a chain is handed over in.  Nothing here touches a device.

The buffer, in int32 words, every piece starting at a multiple of 4 words:
    per stage sa1..sa4:   inds (B, M) | centres (B, M, 3) f32 | ball-query idx (B, M, S) | [row-plan state] |
                          [CSR offsets (B, n_src + 1) | CSR order (B, M * S)]        (CSR: the stages with features, 2..4)
    per FP module:        3-NN weight (B, n, 3) f32 | idx (B, n, 3) | CSR offsets (B, m + 1) | CSR order (B, 3 n)
    the extra level:      inds (B, n)
"""
from typing import Any, NamedTuple, Optional, Tuple

import torch


# ---- layout: word offsets -----------------------------------------------------------------------------------------------

class StageSlot(NamedTuple):
    name: str
    M: int                          # centres per scene
    S: int                          # ball size
    n_src: int                      # points per scene the stage samples from
    inds: int
    xyz: int
    idx: int
    plan: Optional[int]             # the row plan's state, where the stage was planned at launch time
    csr_offsets: Optional[int]
    csr_order: Optional[int]


class FPSlot(NamedTuple):
    unknown: int                    # index of the stage whose centres are interpolated onto ...
    known: int                      # ... from this stage's
    n: int
    m: int
    weight: int
    idx: int
    csr_offsets: int
    csr_order: int


class ExtraSlot(NamedTuple):
    name: str
    n: int
    inds: int


class ChainLayout(NamedTuple):
    total: int
    stages: Tuple[StageSlot, ...]
    fps: Tuple[FPSlot, ...]
    extra: Optional[ExtraSlot]
    plan_group: int                 # sa_fused.PLAN_GROUP when the chain was launched: the group size its plans were made with


def _r4(n):
    return (n + 3) // 4 * 4


def chain_layout(B, n_points, stages, planned, plan_words, fp_pairs, extra, plan_group):
    """stages ((name, M, S), ...); planned[i]: stage i gets a row plan (sa_fused.plan_static_ok, asked by the caller at launch
    time) of plan_words[i] words (sum(sa_fused.plan_words)); fp_pairs ((unknown stage, known stage), ...); extra (name, n) |
    None -> ChainLayout"""
    end = 0

    def piece(words):
        nonlocal end
        at, end = end, end + words
        return at

    slots, n_src = [], n_points
    for i, (name, M, S) in enumerate(stages):
        P = B * M * S
        inds, xyz, idx = piece(_r4(B * M)), piece(_r4(B * M * 3)), piece(_r4(P))
        plan = piece(plan_words[i]) if planned[i] else None
        # stages with features: the CSR "which grouped positions read point k" of their backward
        offsets, order = (piece(_r4(B * (n_src + 1))), piece(_r4(P))) if i > 0 else (None, None)
        slots.append(StageSlot(name, M, S, n_src, inds, xyz, idx, plan, offsets, order))
        n_src = M
    fps = []
    for u, k in fp_pairs:
        n, m = slots[u].M, slots[k].M
        fps.append(FPSlot(u, k, n, m, piece(_r4(B * n * 3)), piece(_r4(B * n * 3)), piece(_r4(B * (m + 1))),
                          piece(_r4(B * n * 3))))
    if extra is not None:
        extra = ExtraSlot(extra[0], extra[1], piece(_r4(B * extra[1])))
    return ChainLayout(end, tuple(slots), tuple(fps), extra, plan_group)


# ---- views of a filled (or to be filled) buffer ---------------------------------------------------------------------------

class Csr(NamedTuple):
    offsets: Any
    order: Any
    space: Optional[Tuple[int, int]]        # the row space it was built in: None (every row) | (goff address, group size)


class StageAhead(NamedTuple):
    centres: Any                    # (B, M, 3) f32
    idx: Any                        # (B, M, S) i32
    plan_state: Any                 # flat i32 (sa_fused.plan_views) | None
    csr: Optional[Csr]
    inds: Any                       # (B, M) i32 | None in the record that rides on this very tensor (no reference cycle)
    planned: bool                   # the plan was made, and the CSR built under it (a planned stage = training)


class FPAhead(NamedTuple):
    unknown: Any                    # the unknown / known stage's `centres`, the very tensors (a module finds its record by
    known: Any                      # identity); unknown is None in the record that rides on it (no reference cycle)
    weight: Any                     # (B, n, 3) f32
    idx: Any                        # (B, n, 3) i32
    csr: Csr


class ChainViews(NamedTuple):
    stages: Tuple[StageAhead, ...]
    fps: Tuple[FPAhead, ...]
    extra: Any                      # (B, n) i32 | None


def _plan_end(layout, i):
    """a plan's state runs up to the piece behind it"""
    slot = layout.stages[i]
    if slot.csr_offsets is not None:
        return slot.csr_offsets
    return layout.stages[i + 1].inds if i + 1 < len(layout.stages) else layout.fps[0].weight


def chain_views(flat, layout, B, planned=None):
    """flat int32 (>= layout.total words), the layout it was (or will be) FILLED with -> ChainViews.  planned[i]: stage i's
    CSR was built under its plan (Ahead.planned of a filled buffer; None: nowhere), which names the CSR's row space."""
    def i32(at, *shape):
        return flat[at:at + _numel(shape)].view(*shape)

    def f32(at, *shape):
        return flat[at:at + _numel(shape)].view(torch.float32).view(*shape)

    stages = []
    for i, s in enumerate(layout.stages):
        state = None if s.plan is None else flat[s.plan:_plan_end(layout, i)]
        under = bool(planned[i]) if planned is not None else False
        csr = None
        if s.csr_offsets is not None and not (under and state is None):
            space = (state.data_ptr(), layout.plan_group) if under else None
            csr = Csr(i32(s.csr_offsets, B, s.n_src + 1), i32(s.csr_order, B, s.M * s.S), space)
        stages.append(StageAhead(f32(s.xyz, B, s.M, 3), i32(s.idx, B, s.M, s.S), state, csr, i32(s.inds, B, s.M), under))
    fps = tuple(FPAhead(stages[f.unknown].centres, stages[f.known].centres, f32(f.weight, B, f.n, 3), i32(f.idx, B, f.n, 3),
                        Csr(i32(f.csr_offsets, B, f.m + 1), i32(f.csr_order, B, f.n * 3), None)) for f in layout.fps)
    extra = None if layout.extra is None else i32(layout.extra.inds, B, layout.extra.n)
    return ChainViews(tuple(stages), fps, extra)


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


# ---- host records ---------------------------------------------------------------------------------------------------------

class ExtraLevel(NamedTuple):
    name: str
    inds: Any
    event: Any                      # to wait for before reading inds | None: inds is a copy already


class Ahead(NamedTuple):
    """what a chain made ahead of the stages (backbone_module.GROUP_AHEAD)"""
    flat: Any
    event: Any
    layout: ChainLayout             # the one `flat` was filled with: a switch flipped before forward() must not move the pieces
    planned: Tuple[bool, ...]


class ChainPlan(NamedTuple):
    """a sampling chain in flight; the consumer's stream waits for events[i] before it reads inds[i]"""
    key: tuple
    src: Any
    trusted: bool
    inds: Optional[list]            # 4 x (B, npoint) i32 in the plan's persistent buffers | None: taken with `ahead`
    events: list
    extra: Optional[ExtraLevel]
    ahead: Optional[Ahead]


class Head(NamedTuple):
    """rounds [0, rounds) of an sa1 sampling in flight (prefetch_head)"""
    rounds: int
    event: Any
    key: tuple
    trusted: bool
    src: Any


class Tail(NamedTuple):
    """the handed-over state the next resumed chain continues"""
    rounds: int
    key: tuple
    trusted: bool


class Pending(NamedTuple):
    """the arguments of a chain that starts inside the next forward() (prefetch(at_next_forward=True))"""
    pointcloud: Any
    trusted: bool
    small: bool
    group: bool
    resume: bool
