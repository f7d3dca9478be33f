"""Deferred weight gradients, the pure part: what `sa_fused.deferred_wgrads` collects (Target, Crop, Item), where a gradient
may be written behind autograd's back (cat_params / joint_params, grad_target, bias_target_ok, the DistributedDataParallel
registry) and `place()`: where every gradient of one grouped launch lands.  Nothing here allocates device memory or
launches; `sa_fused.deferred_wgrads` executes the plan."""
import typing

import torch

import pointnet2_utils

E16 = pointnet2_utils._load_ext().E16          # _JointRows restores the 16-bit element type on the autograd thread


class Target(typing.NamedTuple):
    """Where a gradient may be written behind autograd's back: ONE parameter from element `off` on (a leaf Parameter, or a row
    range of a packed one), or -- `parts` -- rows r0:r1 of the result to each of several (parameter, off, r0, r1)."""
    param: typing.Optional[torch.nn.Parameter] = None
    off: int = 0
    parts: typing.Optional[list] = None

    @property
    def single(self):
        return self.parts is None

    @property
    def params(self):
        return [self.param] if self.single else [q[0] for q in self.parts]

    def covers(self, n):
        """the whole of one parameter of n elements"""
        return self.single and self.off == 0 and self.param.numel() == n


class Crop(typing.NamedTuple):
    """What a problem stores of its M x N product (omnipq_tn_problem): rows x cols of it, the columns mapped by `rot`
    (0, or rot | split << 8 -- one integer, the C ABI's field).  ld is None: that is the whole matrix, at pitch cols; else it
    is the column range [col0, col0 + cols) of a matrix of pitch ld."""
    rows: int
    cols: int
    rot: int = 0
    col0: int = 0
    ld: typing.Optional[int] = None


class Item(typing.NamedTuple):
    """One collected weight (and bias) gradient: out = crop(dY[P][M]^T X[P][N]), bias = column sums of dY."""
    dY: torch.Tensor
    X: torch.Tensor
    M: int
    N: int
    P: int
    wt: Target
    crop: Crop
    bt: typing.Optional[Target] = None     # the bias' target
    aff: typing.Optional[tuple] = None     # (a, b): X stands for relu(a * X + b)
    blk: typing.Any = None                 # the SA stage's row plan (the positions in use live in device memory)


_ZERO_TAILS = {}


def _with_parts(out, tensors):
    """`out` = the rows of `tensors` one after the other: remember who owns which"""
    parts, r = [], 0
    for t in tensors:
        parts.append((t, r, r + t.shape[0]))
        r += t.shape[0]
    out.omnipq_parts = parts
    return out


def cat_params(tensors, dim=0, pad_to=None):
    """torch.cat of parameters along dim 0 (the output heads of a prediction head share one GEMM) that remembers
    its parts, so that `deferred_wgrads` can hand each part its rows of the joint gradient.  pad_to: append zeros up
    to that many rows in the same launch (a bias vector for a padded GEMM)."""
    assert dim == 0
    rows = sum(t.shape[0] for t in tensors)
    if pad_to is not None and pad_to > rows:
        tail = _ZERO_TAILS.get((tensors[0].device, tensors[0].dtype))
        if tail is None or tail.numel() < pad_to - rows:
            tail = _ZERO_TAILS[(tensors[0].device, tensors[0].dtype)] = torch.zeros(
                max(64, pad_to - rows), device=tensors[0].device, dtype=tensors[0].dtype)
        out = torch.cat(list(tensors) + [tail[:pad_to - rows]], 0)
    else:
        out = torch.cat(tensors, 0)
    return _with_parts(out, tensors)


class _JointRows(torch.autograd.Function):
    """The joint buffer as the concatenation of its parts for autograd: no kernel in either direction (forward returns the
    buffer the parameters already live in, backward hands each parameter its rows of the joint gradient as a view)."""

    @staticmethod
    def forward(ctx, joint, *parts):
        ctx.e16 = E16.dtype
        ctx.meta = [(p.shape, p.shape[0]) for p in parts]
        # inside deferred_wgrads the consumer returns no gradient for the joint matrix: an undefined gradient must stay
        # undefined (the default would hand this node a zero tensor, and every parameter a zero .grad to be added to later)
        ctx.set_materialize_grads(False)
        return joint.view(joint.shape)

    @staticmethod
    def backward(ctx, g):
        E16.select(ctx.e16)
        if g is None:
            return (None,) * (1 + len(ctx.meta))
        out, r = [], 0
        for shape, n in ctx.meta:
            out.append(g[r:r + n].reshape(shape))
            r += n
        return (None, *out)


def joint_params(owner, name, params, pad_to=None):
    """cat_params without the per-step copy: the parameters (the 1x1 output heads of a prediction head, which share one
    GEMM) are re-seated ONCE as row ranges of a joint buffer kept on `owner` -- `param.data` becomes a view of it, so
    optimizer steps, load_state_dict and the EMA update write straight into the joint matrix -- and every later call only
    checks the pointers.  A module moved or copied since (`.to()`, deepcopy) fails the check and is re-seated.  The result
    carries the same `omnipq_parts` as cat_params (deferred weight gradients find their targets) and, outside
    `deferred_wgrads`, routes the joint gradient back to the parameters through autograd as views.
    pad_to: rows of zeros appended once (a bias vector for a padded GEMM)."""
    cache = owner.__dict__.setdefault("_omnipq_joint", {})
    rows = sum(p.shape[0] for p in params)
    total = pad_to if (pad_to is not None and pad_to > rows) else rows
    inner = tuple(params[0].shape[1:])
    width = 1
    for d in inner:
        width *= d
    joint = cache.get(name)

    def seated():
        if joint is None or joint.shape[0] != total or joint.device != params[0].device or joint.dtype != params[0].dtype:
            return False
        off = 0
        for p in params:
            if not p.is_contiguous() or tuple(p.shape[1:]) != inner or \
                    p.data_ptr() != joint.data_ptr() + off * width * joint.element_size():
                return False
            off += p.shape[0]
        return True

    if not seated():
        with torch.no_grad():
            joint = torch.zeros((total,) + inner, device=params[0].device, dtype=params[0].dtype)
            off = 0
            for p in params:
                joint[off:off + p.shape[0]].copy_(p.detach())
                p.data = joint[off:off + p.shape[0]]
                off += p.shape[0]
        cache[name] = joint
    tracked = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    return _with_parts(_JointRows.apply(joint, *params) if tracked else joint, params)


def grad_target(t):
    """Where a gradient of `t` may be written behind autograd's back, or None:
    Target(parameter, element offset)      `t` is a leaf Parameter or a contiguous view of a contiguous one (a row
                                           range of a packed projection weight);
    Target(parts=[(parameter, element offset, r0, r1), ...])
                                           `t` = cat_params(...) of such tensors (each part owns rows r0:r1)."""
    if t is None:
        return None
    if isinstance(t, torch.nn.Parameter):
        return Target(t) if t.is_contiguous() and t.requires_grad else None
    parts = getattr(t, "omnipq_parts", None)
    if parts is not None:
        sub = [(grad_target(q), r0, r1) for q, r0, r1 in parts]
        if all(g is not None and g.single for g, _, _ in sub):
            return Target(parts=[(g.param, g.off, r0, r1) for g, r0, r1 in sub])
        return None
    base = t._base
    if isinstance(base, torch.nn.Parameter) and base.requires_grad and base.is_contiguous() and t.is_contiguous():
        return Target(base, t.storage_offset() - base.storage_offset())
    return None


def bias_target_ok(bt, C, Cp):
    """The kernel adds Cp (padded) column sums: straight into a row range of a packed bias only if nothing is
    padded; whole parameters and concatenations get a scratch vector and take views of it."""
    return bt is not None and (Cp == C or not bt.single or bt.covers(C))


# Parameters of every DistributedDataParallel module that has run a forward pass in this process.  DDP reduces gradients
# from per-parameter autograd hooks; a gradient written behind autograd's back never reaches them, so the ranks would
# silently train on their local gradients.  A global forward pre-hook records DDP-wrapped parameters; deferred_wgrads
# refuses them (use data_parallel.GradientBuckets on the bare module, or stay outside deferred_wgrads under DDP).
_DDP_PARAM_IDS = set()


def _note_ddp(module, _args):
    if isinstance(module, torch.nn.parallel.DistributedDataParallel):
        for p in module.parameters():
            _DDP_PARAM_IDS.add(id(p))


torch.nn.modules.module.register_module_forward_pre_hook(_note_ddp)


def _refuse_ddp(wt):
    if not _DDP_PARAM_IDS or wt is None:
        return
    if any(id(p) in _DDP_PARAM_IDS for p in wt.params):
        raise RuntimeError(
            "sa_fused.deferred_wgrads: this parameter belongs to a DistributedDataParallel module -- its gradient would "
            "bypass DDP's reduction hooks.  Run backward outside deferred_wgrads under DDP, or keep the module bare and "
            "reduce with data_parallel.GradientBuckets")


# ---- placement: where the gradients of ONE grouped launch land ----------------------------------------------------------

class Buffer(typing.NamedTuple):
    kind: str                # "empty" | "zeros" (a clearing launch of its own) | "pooled" (a slice of the zero pool)
    numel: int               # f32 elements
    param: typing.Optional[torch.nn.Parameter] = None      # the parameter it is assigned to, whole; None: scratch


class Span(typing.NamedTuple):
    """elements [off, off + n) of buffer `buf` (an index into Placement.buffers); n is None for a problem's `out`, whose
    extent its rows, columns and pitch tell"""
    buf: int
    off: int = 0
    n: typing.Optional[int] = None


class Problem(typing.NamedTuple):
    """the output fields of one omnipq_tn_problem"""
    out: Span
    out_rows: int
    out_cols: int
    out_ld: int
    rot: int
    colsum: typing.Optional[Span]


class Placement(typing.NamedTuple):
    buffers: list            # [Buffer], in the order they are allocated
    problems: list           # [Problem], one per item
    adds: list               # [(destination Span, source Span)] after the launch: second uses of a weight, then the rows of
                             # a joint result that are a part of some parameter's buffer
    assigns: list            # [(parameter, Span viewed in its shape)] for .grad: whole buffers, then views of scratch results


class _Placer:
    """place()'s state while it goes through the items"""

    def __init__(self, items):
        self.buffers, self.again, self.summed, self.views = [], [], [], []
        self.whole = {}      # id(param) -> (index of the buffer of its shape, offsets written so far)
        # which packed weights are covered completely by the row (or column) ranges collected (q | k,v of a
        # cross-attention, features | coordinates of a hoisted first layer): those buffers need no clearing
        covered = {}
        for it in items:
            if it.wt.single:
                ranges = covered.setdefault(id(it.wt.param), (it.wt.param, {}))[1]
                ranges[(it.wt.off, it.crop.col0)] = it.crop.rows * it.crop.cols
        self.complete = {k for k, (p, v) in covered.items() if sum(v.values()) == p.numel()}

    def new(self, kind, numel, param=None):
        self.buffers.append(Buffer(kind, numel, param))
        return len(self.buffers) - 1

    def buffer_of(self, param, full, pooled=False):
        ent = self.whole.get(id(param))
        if ent is None:
            # a gradient assembled from several row ranges starts from zero unless they cover it; one written
            # whole needs no clearing; small vectors that the kernel ADDS to come from the zero pool
            kind = "empty" if (full or id(param) in self.complete) else "pooled" if pooled else "zeros"
            ent = self.whole[id(param)] = (self.new(kind, param.numel(), param), set())
        return ent

    def piece(self, param, off, src):
        """`src` (rows of a scratch result) is the gradient of param's elements [off, off + src.n)."""
        if off == 0 and src.n == param.numel() and id(param) not in self.whole:
            self.views.append((param, src))
        else:
            ent = self.whole.get(id(param))
            if ent is None:
                ent = self.whole[id(param)] = (self.new("zeros", param.numel(), param), set())
            self.summed.append((Span(ent[0], off, src.n), src))

    def weight(self, wt, crop):
        """-> (where the problem stores, its pitch)"""
        n = crop.rows * crop.cols
        if wt.single and crop.ld is not None:
            # a COLUMN range of the parameter's matrix.  Several problems cover one gradient (the hoisted first layer of
            # an SA stage: features | coordinates)
            buf, seen = self.buffer_of(wt.param, False)
            assert (wt.off, crop.col0) not in seen, "column ranges of one weight must be disjoint"
            seen.add((wt.off, crop.col0))
            return Span(buf, wt.off + crop.col0), crop.ld
        if wt.single:
            buf, seen = self.buffer_of(wt.param, wt.covers(n))
            if wt.off in seen:
                # the same weight used twice in the graph: its second gradient goes to a buffer of its own and
                # is added afterwards (two problems of one grid must not touch the same output)
                extra = Span(self.new("empty", n), 0, n)
                self.again.append((Span(buf, wt.off, n), extra))
                return extra, crop.cols
            seen.add(wt.off)
            return Span(buf, wt.off), crop.cols
        scratch = self.new("empty", n)
        for param, off, r0, r1 in wt.parts:
            self.piece(param, off, Span(scratch, r0 * crop.cols, (r1 - r0) * crop.cols))
        return Span(scratch), crop.cols

    def bias(self, bt, M, cout):
        """-> where the kernel ADDS the M column sums (zero on entry), or None"""
        if bt is None:
            return None
        if bt.single and not bt.covers(cout):
            buf, seen = self.buffer_of(bt.param, False, pooled=True)     # row range of a packed bias (M == cout: nothing padded)
            seen.add(bt.off)
            return Span(buf, bt.off, M)
        scratch = self.new("pooled", M)
        if bt.single:
            self.piece(bt.param, 0, Span(scratch, 0, cout))
        else:
            for param, off, r0, r1 in bt.parts:
                self.piece(param, off, Span(scratch, r0, r1 - r0))
        return Span(scratch, 0, M)


def place(items):
    """Where the gradients of one grouped launch land, from host facts alone (every item's M, targets and crop): a pure
    function, nothing is allocated.  The rules:
      * a parameter whose gradient is written in ranges (rows of a packed q | k,v weight or bias, the two column ranges of
        a hoisted first layer) gets ONE buffer of its shape, assigned whole; it is `empty` if one problem writes all of it
        or the ranges collected in this launch cover it, else cleared (`pooled` if first met as a bias, which the kernel
        adds to; else `zeros`);
      * a range met a second time (a weight used twice in the graph) goes to an `empty` scratch and is added afterwards:
        two problems of one launch never share an output;
      * a joint result (cat_params / joint_params) goes to an `empty` scratch; a part that is a whole parameter without a
        buffer of its own is assigned as a view of it, any other part is added into that parameter's `zeros` buffer;
      * column sums are ADDED by the kernel: into a row range of a packed bias' buffer, else into a `pooled` scratch of M
        elements whose parts are handed out like a joint result's."""
    pl = _Placer(items)
    problems = []
    for it in items:
        out, ld = pl.weight(it.wt, it.crop)
        problems.append(Problem(out, it.crop.rows, it.crop.cols, ld, it.crop.rot, pl.bias(it.bt, it.M, it.crop.rows)))
    # `.grad` order: every whole buffer (in the order first met), then the views of scratch results
    assigns = [(pl.buffers[b].param, Span(b, 0, pl.buffers[b].numel)) for b, _ in pl.whole.values()] + pl.views
    return Placement(pl.buffers, problems, pl.again + pl.summed, assigns)
