"""The prediction heads of PQ_Transformer (reference models/pq_transformer.py:35-121) and their host side: the object head
and the layout-quad head of every decoder stage, their stacks on the row kernels (pointnet2/rows_mlp.py), the decode of their
output rows into `end_points` (csrc/head_ops.hip) and the backward of all stages in grouped launches.

    rows, lin, conv1x1, conv1x1_pair   1x1 convolutions on row-major activations (shared with pq_transformer)
    HEAD_OUTS, QUAD_OUTS               what a decode produces: one row per output, in the kernels' order
    HeadDecode, QuadDecode, DecodePair the decode as autograd nodes; their arguments are marshalled in ONE place each way
    heads_bwd_route, stage_route       how a forward / a stage runs, from flags alone
    predict_pair                       one stage; begin() -> HeadsForward: what one forward pass of the model keeps
    PredictHead, QuadPredictHead       the modules (re-exported by pq_transformer: pickles and state_dict names stay)

Every module switch below exists here only and is read as an attribute of this module when a call needs it.
"""
import ctypes
import os
import sys
import typing

import numpy as np
import torch
from torch import nn

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE), os.path.join(os.path.dirname(_HERE), "pointnet2")):
    if _p not in sys.path:                       # (importable on its own: a pickled head names this module)
        sys.path.append(_p)

import rows_f32  # noqa: E402
import rows_mlp  # noqa: E402
import sa_fused  # noqa: E402
from sa_fused import E16  # noqa: E402


# The 1x1 convolutions of heads, position embeddings and projections are per-point linear layers.  They run
# here on row-major activations (points x channels) through F.linear -- one GEMM with the bias in its
# epilogue -- instead of Conv1d on (B, C, K): same arithmetic, no layout-shuffling copies around every call,
# and the heads' outputs come out directly in the (B, K, C) form the reference produces with .transpose(2, 1).
def rows(x):
    """(B, C, K) -> (B*K, C) rows (a free reshape when x is a transposed view of (B, K, C) data)."""
    B, C, K = x.shape
    return x.transpose(1, 2).reshape(B * K, C)


def lin(x2d, conv):
    """kernel-size-1 Conv1d applied to rows: (N, C_in) -> (N, C_out)"""
    stack = [rows_mlp.Layer(conv.weight, conv.bias)]
    if rows_mlp.usable(x2d, stack, conv.training):
        return rows_mlp.run(x2d, stack, conv.training)          # bf16 MFMA GEMM, weight gradient deferrable
    return rows_f32.linear(x2d, conv.weight, conv.bias)         # f32 mode: hand-written split-f32 GEMM on a GPU


def conv1x1_pair(xa, conv_a, xb, conv_b):
    """`conv1x1` of two independent inputs through two independent layers; on the row kernels their GEMMs share a launch
    each way (rows_mlp.run_pair)."""
    ra, rb = rows(xa), rows(xb)
    sa, sb = [rows_mlp.Layer(conv_a.weight, conv_a.bias)], [rows_mlp.Layer(conv_b.weight, conv_b.bias)]
    if stacks_paired(conv_a.training == conv_b.training, rows_mlp.usable(ra, sa, conv_a.training),
                     rows_mlp.usable(rb, sb, conv_b.training)):
        ya, yb = rows_mlp.run_pair(ra, sa, rb, sb, conv_a.training)
    else:
        ya, yb = lin(ra, conv_a), lin(rb, conv_b)
    (Ba, _, Ka), (Bb, _, Kb) = xa.shape, xb.shape
    return ya.view(Ba, Ka, -1).transpose(1, 2), yb.view(Bb, Kb, -1).transpose(1, 2)


def conv1x1(x, conv):
    """(B, C_in, K) -> (B, C_out, K), as a transposed view of the row-major result."""
    B, _, K = x.shape
    return lin(rows(x), conv).view(B, K, -1).transpose(1, 2)


# ---- switches -----------------------------------------------------------------------------------------------------------
_JOINT_HEADS = True
# The prediction heads' stacks on the inference chain (rows_mlp.EVAL_CHAIN).  Measured faster (profiles/
# rows_infer_ab.txt: head pair) and shipped OFF: tests/test_gpu_decoder.py pins that the eval forward sends the heads' GEMMs out as
# pair launches and that paired and single heads give the same bits, and the chain rounds a hidden activation once where the
# stored route rounds it twice.  On: both head_stack and head_stack_pair opt in.
_HEAD_EVAL_CHAIN = False
_FUSED_DECODE = True       # False: the op-by-op decode of the reference (tests compare the two)
_PAIR_DECODE = True        # toggled by tests/test_gpu_decoder.py to compare with the separate launches
_XYZ_SINK = True
_PAIR_STACKS = True        # two readers: the head pair of a stage and the query-projection pair (conv1x1_pair)
# The pair decode also writes the next layer's query positions as the padded 16-bit rows its position embedding starts from
# (omnipq_decode_pair_pos16), attached to the positions the way rows_mlp._input_rows looks for a prepared operand: no
# omnipq_pad_rows_e16 launch on the query side.  False: rows_mlp converts them, as before -- the same bits.
_POS_ROWS16 = True
_POS_KPAD = 32            # three coordinates at the row GEMMs' operand width (rows_mlp: cin rounded up to 32)
# The backward of the prediction heads of ALL stages in grouped launches.  Every output of a stage's heads goes to the loss and
# nowhere else -- the centres that feed the next layer's position embedding are detached, the base positions' gradient goes to
# the sink -- so when backward starts the output gradients of all stages exist, yet autograd runs stage i's six small launches
# (decode backward, three data-gradient GEMMs, two BatchNorm applies, each a fraction of the chip) between decoder layers
# i + 1 and i.  With the switch on, a stage's forward runs where and as it does otherwise, but outside autograd: what it would
# save is kept on a HeadsGroup, and after the last stage ONE node (HeadsJoint) puts aliases of all stages' outputs into
# end_points.  Its backward has every output gradient at once: one grouped decode backward per four stages
# (omnipq_decode_pair_group_bwd), then the stacks' backward programs of all stages in lockstep, every round one grid
# (rows_mlp._lockstep, omnipq_pair_group).  Same arithmetic per problem, same bits.  False: the per-stage nodes.
_HEADS_BWD_GROUP = True
_HEADS_GROUP_MAX = 7         # stages; two stacks each: the 14 launches a group holds (csrc/common.h: kHeldMax)


# ---- routes: pure functions of flags (no tensor, no launch; the switches are read when they are called) -------------------
def heads_bwd_route(stages, pair_stacks, pair_decode, fused_decode, cuda, training, grad, world, force_collectives):
    """"group" | "stage": how the prediction heads' backward runs, from flags alone (no tensor, no launch; the switch is read
    now).  The grouped route is the pair route of every stage (its three switches, a GPU, training with grad) without a
    statistics exchange (one rank, no forced collectives: the exchange is made per pair) for as many stages as a group
    holds."""
    if not (_HEADS_BWD_GROUP and pair_stacks and pair_decode and fused_decode and cuda and training and grad):
        return "stage"
    if world != 1 or force_collectives or not (1 <= stages <= _HEADS_GROUP_MAX):
        return "stage"
    return "group"


def stage_route(grouped, like_first, cuda, usable_a, usable_b, head_training, quad_training, base_grad, has_sink):
    """How ONE stage runs:
    "group"   the pair route taped, its backward left to the joint node of all stages: the forward chose the grouped route
              (`grouped`: heads_bwd_route, which has looked at the switches, the GPU, training and grad), both heads train on
              the row kernels, the base positions' gradient has somewhere to go (none needed, or a sink), and the stage has
              the geometry and the sink of the group's first stage (`like_first`)
    "pair"    both stacks on the row kernels (launched pairwise where `stacks_paired`), one pair decode
    "stacks"  a stack off the row kernels: each stack by itself (head_stack_pair), then each head's own `finish` -- which
              decodes fused or op by op as its rows allow; where BOTH came out as 16-bit rows all the same (torch's
              autocast), the pair decode takes them
    "single"  no pair decode (a switch, or no GPU): each head by itself"""
    if grouped and head_training and quad_training and not (base_grad and not has_sink) and usable_a and usable_b and like_first:
        return "group"
    if not (_PAIR_DECODE and _FUSED_DECODE and cuda):
        return "single"
    return "pair" if (usable_a and usable_b) else "stacks"


def stacks_paired(same_mode, usable_a, usable_b):
    """whether two stacks go out as one node whose GEMMs share launches (rows_mlp.run_pair)"""
    return bool(_PAIR_STACKS and same_mode and usable_a and usable_b)


# ---- the stacks -----------------------------------------------------------------------------------------------------------
class StackProblem(typing.NamedTuple):
    """One prediction head's stack for rows_mlp: input rows, the three layers (the output layer's bias is seated by
    _head_bias), the joint output weight, and whether the row kernels take it."""
    x: torch.Tensor
    stack: list
    w: torch.Tensor
    usable: bool


def _rows_of(heads):
    out, r = [], 0
    for h in heads:
        out.append((h, r, r + h.weight.shape[0]))
        r += h.weight.shape[0]
    return out


def _head_problem(self, net, heads, net_rows=None):
    """-> StackProblem; the ONE place the heads ask rows_mlp.usable"""
    B, K = net.shape[0], net.shape[2]
    x = rows(net) if net_rows is None else net_rows.reshape(B * K, -1)
    # the output heads' weights / biases live as row ranges of one joint matrix / vector (re-seated once, then only pointer
    # checks): the concatenation every step cost two copy launches per prediction head
    if _JOINT_HEADS and net.is_cuda:
        w = sa_fused.joint_params(self, "w", [h.weight for h in heads]).squeeze(-1)
        w.omnipq_parts = [(h.weight, r0, r1) for (_, r0, r1), h in zip(_rows_of(heads), heads)]
        w.omnipq_persistent = True                       # the joint buffer's address outlives the step: weight arena
    else:
        w = sa_fused.cat_params([h.weight.squeeze(-1) for h in heads])
    stack = [rows_mlp.Layer(self.conv1.weight, self.conv1.bias, self.bn1),
             rows_mlp.Layer(self.conv2.weight, self.conv2.bias, self.bn2), rows_mlp.Layer(w, None)]
    return StackProblem(x, stack, w, bool(rows_mlp.usable(x, stack, self.training)))


def _head_bias(self, stack, heads, w, raw, on_gpu):
    """The output layer's joint bias (zero-padded to the kernels' width with `raw`).  ONE seated buffer serves both modes:
    it is always padded, the unpadded form is its leading view (two buffers would un-seat each other at every call)."""
    width = w.shape[0]
    padded = (width + 31) // 32 * 32
    if _JOINT_HEADS and on_gpu:
        b = sa_fused.joint_params(self, "b", [h.bias for h in heads], pad_to=padded)
        if not raw and padded != width:
            parts = b.omnipq_parts
            b = b[:width]
            b.omnipq_parts = parts
        stack[2].bias = b
    else:
        stack[2].bias = sa_fused.cat_params([h.bias for h in heads], pad_to=padded if raw else None)


def seat_head_parameters(head):
    """Move the 1x1 output heads' weights and biases of a prediction head into their joint buffers NOW (sa_fused.joint_params
    does it lazily inside the first forward otherwise).  Anything that records parameter storage -- a captured hipGraph,
    flattened / bucketed gradient views, an optimizer's foreach lists -- must be built after this; PQ_Transformer calls it
    for every head whenever the module is moved (`.to()`, `.cuda()`), so only code that holds raw pointers across such a
    move has to care."""
    heads = head.heads()
    if not (_JOINT_HEADS and heads[0].weight.is_cuda):
        return
    w = sa_fused.joint_params(head, "w", [h.weight for h in heads])
    width = w.shape[0]
    sa_fused.joint_params(head, "b", [h.bias for h in heads], pad_to=(width + 31) // 32 * 32)


def head_stack(self, net, heads, net_rows=None, raw=False, problem=None):
    """Trunk (2 x Conv1d+BN+ReLU) and every 1x1 output head of a prediction head on (B, C, K) features.
    The output heads share one GEMM over their concatenated weights.  -> list of (B, K, C_h) tensors, i.e.
    already in the layout the reference reaches with `.transpose(2, 1)`.
    net_rows: the same features as (B, K, C) data in another dtype (the decoder's bf16 rows), used instead of
    `net` when given -- the kernels want bf16 rows anyway, this saves the cast forth and back.
    problem: the StackProblem of these arguments, where the caller has it already."""
    x, stack, w, usable = problem or _head_problem(self, net, heads, net_rows)
    B, K = net.shape[0], net.shape[2]
    if usable:
        # hand-written MFMA / BN kernels; with `raw` the consumer takes the kernels' zero-padded rows as they are
        _head_bias(self, stack, heads, w, raw, net.is_cuda)
        y = rows_mlp.run(x, stack, self.training, padded=raw, eval_chain=_HEAD_EVAL_CHAIN)
    else:
        x = rows_f32.bn_act(lin(x, self.conv1), self.bn1)
        x = rows_f32.bn_act(lin(x, self.conv2), self.bn2)
        y = rows_f32.linear(x, w, torch.cat([h.bias for h in heads], 0))
    if raw:
        return y                                         # (B*K, >= sum of head widths) rows
    return list(torch.split(y.view(B, K, -1), [h.out_channels for h in heads], dim=2))


def head_stack_pair(head, quad_head, net, net_q, rows_a=None, rows_b=None, problems=None, taped=False):
    """`head_stack(..., raw=True)` of the object and the quad head of one decoder stage; on the row kernels the two stacks
    run as one node whose GEMMs go out pairwise (rows_mlp.run_pair: each alone covers less than a workgroup per CU).
    taped (a grouped stage: two training stacks on the row kernels): the same forward outside autograd -> (ya, yb, tape)."""
    pa, pb = problems or (_head_problem(head, net, head.heads(), rows_a),
                          _head_problem(quad_head, net_q, quad_head.heads(), rows_b))
    if taped or stacks_paired(head.training == quad_head.training, pa.usable, pb.usable):
        _head_bias(head, pa.stack, head.heads(), pa.w, True, net.is_cuda)
        _head_bias(quad_head, pb.stack, quad_head.heads(), pb.w, True, net_q.is_cuda)
        if taped:
            return rows_mlp.tape_pair(pa.x, pa.stack, pb.x, pb.stack, True, padded=True)
        return rows_mlp.run_pair(pa.x, pa.stack, pb.x, pb.stack, head.training, padded=True, eval_chain=_HEAD_EVAL_CHAIN)
    return (head_stack(head, net, head.heads(), rows_a, raw=True, problem=pa),
            head_stack(quad_head, net_q, quad_head.heads(), rows_b, raw=True, problem=pb))


# ---- what a decode produces: one row per output, in the kernels' order (csrc/head_ops.hip: HeadOut, QuadOut) ---------------
class Out(typing.NamedTuple):
    key: str                     # its end_points key, behind the stage's prefix
    shape: typing.Callable       # (nh, ns, ncls) -> the shape behind (B, K)
    f32: bool                    # float32; otherwise the step's 16-bit element type
    n2: int                      # the second-level width the backward kernels read its gradient with


HEAD_OUTS = (Out("objectness_scores", lambda nh, ns, ncls: (2,), False, 1),
             Out("center", lambda nh, ns, ncls: (3,), True, 1),
             Out("heading_scores", lambda nh, ns, ncls: (nh,), False, 1),
             Out("heading_residuals_normalized", lambda nh, ns, ncls: (nh,), False, 1),
             Out("heading_residuals", lambda nh, ns, ncls: (nh,), False, 1),
             Out("size_scores", lambda nh, ns, ncls: (ns,), False, 1),
             Out("size_residuals_normalized", lambda nh, ns, ncls: (ns, 3), False, 3),
             Out("size_residuals", lambda nh, ns, ncls: (ns, 3), True, 3),
             Out("pred_size", lambda nh, ns, ncls: (3,), True, 1),
             Out("sem_cls_scores", lambda nh, ns, ncls: (ncls,), False, 1))
QUAD_OUTS = (Out("quad_scores", lambda nh, ns, ncls: (2,), False, 1),
             Out("quad_center", lambda nh, ns, ncls: (3,), True, 1),
             Out("normal_vector", lambda nh, ns, ncls: (3,), False, 1),
             Out("quad_size", lambda nh, ns, ncls: (2,), False, 1))
PAIR_OUTS = HEAD_OUTS + QUAD_OUTS
_NH, _NP = len(HEAD_OUTS), len(PAIR_OUTS)


def _alloc(table, B, K, dev, nh=0, ns=0, ncls=0):
    return [torch.empty((B, K) + o.shape(nh, ns, ncls), device=dev, dtype=torch.float32 if o.f32 else E16.dtype)
            for o in table]


def _publish(table, outs, end_points, prefix):
    for o, val in zip(table, outs):
        end_points[f'{prefix}{o.key}'] = val


# ---- one marshalling of a decode's arguments ------------------------------------------------------------------------------
def _ptr_array(values):
    return (ctypes.c_void_p * len(values))(*values)


def _int_array(values):
    return (ctypes.c_int * len(values))(*values)


def _one(tensors):
    """a stage's tensor as an argument of a single-stage entry point"""
    return sa_fused._p(tensors[0])


def _each(tensors):
    """the stages' tensors as an argument of the n-stage entry point"""
    return _ptr_array([None if t is None else t.data_ptr() for t in tensors])


def _f32(base_xyz):
    """base positions as the kernels read them (the caller keeps the result alive through the launch)"""
    return base_xyz.detach().float().contiguous()


def _forward_half(table, y, base, width, nh=0, ns=0, ncls=0):
    """One head's side of a forward entry point, base = _f32(base positions) -> (outputs, (rows, rows per scene), (y, ldy,
    base), output pointers)"""
    B, K, _ = base.shape
    assert y.dtype == E16.dtype and y.stride(1) == 1 and y.shape[0] == B * K and y.shape[1] >= width
    outs = _alloc(table, B, K, y.device, nh, ns, ncls)
    return outs, (B * K, K), (sa_fused._p(y), y.stride(0), sa_fused._p(base)), _ptr_array([o.data_ptr() for o in outs])


def _head_forward(y, base, means, nh, ns, ncls):
    """-> (outputs, the object head's arguments of a pair forward (a lone omnipq_head_decode takes them without the second,
    K), hr_scale)"""
    outs, dims, src, ptrs = _forward_half(HEAD_OUTS, y, base, 5 + 2 * nh + 4 * ns + ncls, nh, ns, ncls)
    scale = float(np.float32(np.pi / nh))
    return outs, (*dims, nh, ns, ncls, *src, sa_fused._p(means), scale, ptrs), scale


def _quad_forward(y, base):
    """-> (outputs, norm, the quad head's arguments of a pair forward (omnipq_quad_decode: without the second))"""
    outs, dims, src, ptrs = _forward_half(QUAD_OUTS, y, base, 10)
    norm = torch.empty(1, device=y.device, dtype=torch.float32)
    return outs, norm, (*dims, *src, ptrs, sa_fused._p(norm))


def _without_k(args):
    return args[:1] + args[2:]


def _grad_descriptors(gs, n2):
    """(device pointers | None, flat strides [len][4], dtype flags) of incoming gradients of logical shape
    [B][K][n1]([n2]); keeps converted tensors alive through the returned list."""
    ptrs, strides, flags, keep = [], [], [], []
    for g, last in zip(gs, n2):
        if g is None:
            ptrs.append(None)
            strides += [0, 0, 0, 0]
            flags.append(0)
            continue
        if g.dtype not in (torch.float32, E16.dtype):
            g = g.float()
        keep.append(g)
        st = list(g.stride())
        ptrs.append(g.data_ptr())
        strides += st if len(st) == 4 else st + [0]
        flags.append(int(g.dtype == E16.dtype))
    return ptrs, strides, flags, keep


class _Half(typing.NamedTuple):
    """One head's side of one stage's decode backward."""
    y: torch.Tensor
    aux: torch.Tensor            # the mean sizes | the normals' norm
    dy: torch.Tensor
    g: tuple                     # _grad_descriptors of its output gradients


def _half(table, y, aux, gs, R):
    return _Half(y, aux, torch.empty((R, y.shape[1]), device=y.device, dtype=E16.dtype),
                 _grad_descriptors(gs, [o.n2 for o in table]))


def _backward_half(table, halves, lead, scale, col):
    """One head's side of a backward entry point, up to and without its base-position gradient, for one stage (col = _one) or
    for several of the same geometry (col = _each): (rows, rows per scene, ...), y, ldy, means | norm, (hr_scale), gradient
    pointers, strides, (n2), dtype flags, dy, lddy."""
    flat = [[v for h in halves for v in h.g[i]] for i in range(3)]
    n2 = (_int_array([o.n2 for o in table]),) if table is HEAD_OUTS else ()
    return (*lead, col([h.y for h in halves]), halves[0].y.stride(0), col([h.aux for h in halves]), *scale,
            _ptr_array(flat[0]), _int_array(flat[1]), *n2, _int_array(flat[2]), col([h.dy for h in halves]),
            halves[0].dy.stride(0))


def _pair_backward(stages, geom, sink, need_dbh, need_dbq, grouped):
    """The decode backward of one stage (omnipq_decode_pair_bwd) or of several of one geometry (grouped:
    omnipq_decode_pair_group_bwd, whatever their number).  stages: [((yh, means, yq, norm), its fourteen output gradients)];
    need_dbq: per stage.  The object base positions' gradient is added into the sink where there is one (the first use
    allocates it, every later one accumulates) and returned otherwise.
    -> (dyh per stage, dyq per stage, dbh | None, dbq per stage)"""
    B, K, nh, ns, ncls, scale, Bq, Kq = geom
    yh0 = stages[0][0][0]
    f32 = dict(device=yh0.device, dtype=torch.float32)
    hs = [_half(HEAD_OUTS, yh, means, g[:_NH], B * K) for (yh, means, _, _), g in stages]
    qs = [_half(QUAD_OUTS, yq, norm, g[_NH:_NP], Bq * Kq) for (_, _, yq, norm), g in stages]
    dbq = [torch.empty((Bq, Kq, 3), **f32) if need else None for need in need_dbq]
    dbh, into, acc = None, None, 0
    if sink is not None and need_dbh:
        acc = int(sink.buf is not None)
        if not acc:
            sink.buf = torch.empty((B, K, 3), **f32)
        into = sink.buf
    elif need_dbh:
        assert not grouped                                   # (stage_route: a grouped stage needs no gradient there, or a sink)
        dbh = into = torch.empty((B, K, 3), **f32)
    col = _each if grouped else _one
    head = _backward_half(HEAD_OUTS, hs, (B * K, K, nh, ns, ncls), (scale,), col)
    quad = _backward_half(QUAD_OUTS, qs, (Bq * Kq, Kq), (), col) + (col(dbq),)
    if grouped:
        sa_fused._call(sa_fused._lib.omnipq_decode_pair_group_bwd, yh0, len(stages), *head, None, *quad, sa_fused._p(into), acc)
    else:
        sa_fused._call(sa_fused._lib.omnipq_decode_pair_bwd, yh0, *head, sa_fused._p(into), *quad, acc)
    return [h.dy for h in hs], [q.dy for q in qs], dbh, dbq


class HeadDecode(torch.autograd.Function):
    """Everything between the object head's output GEMM and its `end_points` entries (reference :35-59, :86-89) in
    one launch, and the gradient of all of it in another (csrc/head_ops.hip): y (B*K, 5 + 2 nh + 4 ns + ncls) bf16
    rows -> objectness, center (= offset + base_xyz), heading scores / residuals (normalised and scaled), size
    scores / residuals (normalised and times the mean sizes), pred_size (arg-max cluster), semantic scores.
    Same values and dtypes as the op-by-op composition below it in `decode_scores`."""

    @staticmethod
    def forward(ctx, y, base_xyz, means, nh, ns, ncls):
        ctx.e16 = E16.dtype
        base = _f32(base_xyz)
        outs, args, scale = _head_forward(y, base, means, nh, ns, ncls)
        sa_fused._call(sa_fused._lib.omnipq_head_decode, y, *_without_k(args))
        ctx.save_for_backward(y, means)
        ctx.geom = (*base_xyz.shape[:2], nh, ns, ncls, scale)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        E16.select(ctx.e16)
        y, means = ctx.saved_tensors
        B, K, nh, ns, ncls, scale = ctx.geom
        half = _half(HEAD_OUTS, y, means, gs, B * K)
        dbase = torch.empty((B, K, 3), device=y.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        sa_fused._call(sa_fused._lib.omnipq_head_decode_bwd, y,
                       *_backward_half(HEAD_OUTS, [half], (B * K, K, nh, ns, ncls), (scale,), _one), sa_fused._p(dbase))
        return half.dy, dbase, None, None, None, None


class QuadDecode(torch.autograd.Function):
    """The quad head after its output GEMM (reference :105-120) in one launch each way: y (B*K, 10) bf16 rows ->
    quad_scores, quad_center (= offset + base_xyz), normal_vector (divided by the 2-norm of the WHOLE tensor, as the
    reference does), quad_size."""

    @staticmethod
    def forward(ctx, y, base_xyz):
        ctx.e16 = E16.dtype
        base = _f32(base_xyz)
        outs, norm, args = _quad_forward(y, base)
        sa_fused._call(sa_fused._lib.omnipq_quad_decode, y, *_without_k(args))
        ctx.save_for_backward(y, norm)
        ctx.geom = tuple(base_xyz.shape[:2])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        E16.select(ctx.e16)
        y, norm = ctx.saved_tensors
        B, K = ctx.geom
        half = _half(QUAD_OUTS, y, norm, gs, B * K)
        dbase = torch.empty((B, K, 3), device=y.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        sa_fused._call(sa_fused._lib.omnipq_quad_decode_bwd, y, *_backward_half(QUAD_OUTS, [half], (B * K, K), (), _one),
                       sa_fused._p(dbase))
        return half.dy, dbase


class XyzGradSink:
    """Where the decodes of all stages leave the gradient of their common base positions (`cluster_xyz`: every stage of
    the reference decodes against it, models/pq_transformer.py:230, :262): the kernels add into one buffer instead of
    autograd adding seven tensors one launch at a time.  `SinkFlush` hands the sum to `cluster_xyz`."""

    def __init__(self):
        self.buf = None


class SinkFlush(torch.autograd.Function):
    """feat -> an alias of feat.  Everything that decodes against `xyz` through `sink` must be computed from the alias:
    then this node's backward runs after all of theirs, and returns the sink's sum as the gradient of `xyz`."""

    @staticmethod
    def forward(ctx, feat, xyz, sink):
        ctx.e16 = E16.dtype
        ctx.sink = sink
        return feat.view_as(feat)

    @staticmethod
    def backward(ctx, g):
        E16.select(ctx.e16)
        buf, ctx.sink.buf = ctx.sink.buf, None
        return g, buf, None


def _decode_pair(yh, base_h, means, nh, ns, ncls, yq, base_q, want_pos, pos_kpad):
    """The pair decode's forward launch -> (the fourteen outputs (+ pos (+ pos16)), what backward needs of it: the saved
    tensors (yh, means, yq, norm) and the geometry)"""
    bh, bq = _f32(base_h), _f32(base_q)
    outs_h, head, scale = _head_forward(yh, bh, means, nh, ns, ncls)
    outs_q, norm, quad = _quad_forward(yq, bq)
    (B, K, _), (Bq, Kq, _) = base_h.shape, base_q.shape
    dev = yh.device
    pos = torch.empty((B, K + Kq, 3), device=dev, dtype=torch.float32) if (want_pos and B == Bq) else None
    # pos_kpad: the positions also as the 16-bit rows, padded to pos_kpad columns, that the next layer's position
    # embedding starts from (a sixteenth output, without gradient)
    pos16 = torch.empty((B * (K + Kq), pos_kpad), device=dev, dtype=E16.dtype) if (pos is not None and pos_kpad >= 3) else None
    if pos16 is None:
        sa_fused._call(sa_fused._lib.omnipq_decode_pair, yh, *head, *quad, sa_fused._p(pos))
    else:
        sa_fused._call(sa_fused._lib.omnipq_decode_pair_pos16, yh, *head, *quad, sa_fused._p(pos), sa_fused._p(pos16), pos_kpad)
    extra = () if pos is None else (pos,) if pos16 is None else (pos, pos16)
    return tuple(outs_h) + tuple(outs_q) + extra, (yh, means, yq, norm), (B, K, nh, ns, ncls, scale, Bq, Kq)


class DecodePair(torch.autograd.Function):
    """`HeadDecode` and `QuadDecode` of one decoder stage in ONE launch each way (csrc/head_ops.hip, decode_pair): the two
    heads are independent and each decode is a few microseconds of work, so the pair costs one launch instead of two.
    Outputs: the ten of `HeadDecode`, then the four of `QuadDecode`, bit for bit; with `want_pos` a fifteenth: both
    centres side by side per scene, (B, K + Kq, 3) f32 without gradient -- the next layer's query positions.
    sink (XyzGradSink | None): the gradient of `base_h` is added into the sink instead of being returned."""

    @staticmethod
    def forward(ctx, yh, base_h, means, nh, ns, ncls, yq, base_q, sink=None, want_pos=False, pos_kpad=0):
        ctx.e16 = E16.dtype
        outs, saved, ctx.geom = _decode_pair(yh, base_h, means, nh, ns, ncls, yq, base_q, want_pos, pos_kpad)
        ctx.save_for_backward(*saved)
        ctx.sink = sink
        # (an output nobody differentiates -- always the positions, with a supervised loss some of the others -- arrives in
        # backward as None, which _grad_descriptors passes on as a null pointer, instead of as a zero tensor autograd fills)
        ctx.set_materialize_grads(False)
        if len(outs) > _NP:
            ctx.mark_non_differentiable(*outs[_NP:])
        return outs

    @staticmethod
    def backward(ctx, *gs):
        E16.select(ctx.e16)
        nig = ctx.needs_input_grad
        (dyh,), (dyq,), dbh, (dbq,) = _pair_backward([(ctx.saved_tensors, gs)], ctx.geom, ctx.sink, nig[1], [nig[7]], False)
        return dyh, dbh, None, None, None, None, dyq, dbq, None, None, None


# ---- one stage, one forward pass ------------------------------------------------------------------------------------------
def predict_pair(head, quad_head, net, net_q, base_xyz, base_xyz_q, end_points, prefix, rows=None, rows_q=None,
                 sink=None, want_pos=False, group=None):
    """`head(net, ...)` then `quad_head(net_q, ...)` of one decoder stage (reference models/pq_transformer.py:230-233,
    :262-267), by the stage's route (stage_route); with the fused decode both heads' tails share one launch each way.
    group (HeadsGroup | None): the stage's backward is left to the joint node of all stages (see HeadsGroup).
    -> (object centres, quad centres, end_points, both centres as one (B, K + Kq, 3) tensor | None)."""
    # the facts of the stage, gathered here and nowhere else
    pa = _head_problem(head, net, head.heads(), rows)
    pb = _head_problem(quad_head, net_q, quad_head.heads(), rows_q)
    nh, ns, ncls = head.num_heading_bin, head.num_size_cluster, head.num_class
    geom = (net.shape[0], net.shape[2], nh, ns, ncls, net_q.shape[0], net_q.shape[2], pa.w.shape[0], pb.w.shape[0])
    route = stage_route(group is not None, group is not None and group.takes(geom, sink), net.is_cuda, pa.usable, pb.usable,
                        head.training, quad_head.training, base_xyz.requires_grad, sink is not None)
    if route == "single":
        center, _, end_points = head(net, base_xyz=base_xyz, end_points=end_points, prefix=prefix, net_rows=rows, problem=pa)
        center_q, _, end_points = quad_head(net_q, base_xyz=base_xyz_q, end_points=end_points, prefix=prefix,
                                            net_rows=rows_q, problem=pb)
        return center, center_q, end_points, None
    # "pair" and "group" are ONE body -- the two stacks, then the pair decode -- under autograd or taped: what the nodes of a
    # taped stage would save stays with the group, whose joint node runs the backward of all stages
    taped = route == "group"
    yh, yq, *tape = head_stack_pair(head, quad_head, net, net_q, rows, rows_q, problems=(pa, pb), taped=taped)
    if route == "stacks" and not (_fused_rows(yh) and _fused_rows(yq)):
        center, _, end_points = head.finish(yh, net, base_xyz, end_points, prefix)
        center_q, _, end_points = quad_head.finish(yq, net_q, base_xyz_q, end_points, prefix)
        return center, center_q, end_points, None
    args = (yh, base_xyz, head._mean_sizes(net.device), nh, ns, ncls, yq, base_xyz_q)
    tail = (want_pos, _POS_KPAD if (want_pos and _POS_ROWS16) else 0)
    if taped:
        outs, saved, decode_geom = _decode_pair(*args, *tail)
        group.add(geom, sink, HeadsGroup.Stage(prefix, pa.x, pb.x, base_xyz_q, tape[0], saved, decode_geom, outs[:_NP]))
    else:
        outs = DecodePair.apply(*args, sink, *tail)
    _publish(PAIR_OUTS, outs, end_points, prefix)
    pos = outs[_NP] if len(outs) > _NP else None
    if len(outs) > _NP + 1:
        # (here, not inside DecodePair.forward: attributes set there need not survive `apply`)
        rows2d = pos.view(-1, 3)
        rows2d.omnipq_rows_in = (rows2d._version, outs[_NP + 1])
        pos.omnipq_rows2d = rows2d
    return outs[1], outs[_NH + 1], end_points, pos


class HeadsGroup:
    """What the grouped stages of ONE forward pass keep for their joint backward (see _HEADS_BWD_GROUP)."""

    class Stage(typing.NamedTuple):
        prefix: str
        xa: torch.Tensor
        xb: torch.Tensor
        base_q: torch.Tensor
        tape: object             # rows_mlp.tape_pair's
        saved: tuple             # the decode's (yh, means, yq, norm)
        decode_geom: tuple
        outs: tuple

    def __init__(self):
        self.stages, self.sink, self.geom = [], None, None

    def takes(self, geom, sink):
        """one grouped decode takes stages of the same shapes and the same sink only"""
        return not self.stages or (geom == self.geom and sink is self.sink)

    def add(self, geom, sink, stage):
        self.geom, self.sink = geom, sink
        self.stages.append(stage)

    def finish(self, end_points):
        """After the last stage: the joint node, and its aliases of every grouped stage's outputs into end_points."""
        if not self.stages:
            return
        flat = []
        for st in self.stages:
            flat += [st.xa, st.xb, st.base_q, *st.tape.params_a, *st.tape.params_b]
        outs = HeadsJoint.apply(self, *flat)
        for s, st in enumerate(self.stages):
            _publish(PAIR_OUTS, outs[_NP * s:_NP * (s + 1)], end_points, st.prefix)


class HeadsJoint(torch.autograd.Function):
    """(group, per stage: object rows, quad rows, quad base positions, the two stacks' parameters) -> aliases of the fourteen
    decode outputs of every stage.  backward: see _HEADS_BWD_GROUP; a stage none of whose outputs carries a gradient is left
    out of the group."""

    @staticmethod
    def forward(ctx, group, *flat):
        ctx.e16 = E16.dtype
        ctx.group = group
        ctx.set_materialize_grads(False)
        return tuple(o.view_as(o) for st in group.stages for o in st.outs)

    @staticmethod
    def backward(ctx, *gs):
        E16.select(ctx.e16)
        group, nig = ctx.group, ctx.needs_input_grad
        grads = [None] * len(nig)
        live, first = [], 1                                  # (stage, its gradients, index of its first input)
        for s, st in enumerate(group.stages):
            g = gs[_NP * s:_NP * (s + 1)]
            if any(x is not None for x in g):
                live.append((st, g, first))
            first += 3 + len(st.tape.params_a) + len(st.tape.params_b)
        live.reverse()                                       # the order of the per-stage nodes: the last stage first
        if not live:
            return tuple(grads)
        n = len(live)
        dyh, dyq, _, dbq = _pair_backward([(st.saved, g) for st, g, _ in live], live[0][0].decode_geom, group.sink,
                                          group.sink is not None, [nig[first + 2] for _, _, first in live], True)
        programs = []
        for j, (st, _, first) in enumerate(live):
            na, nb = len(st.tape.params_a), len(st.tape.params_b)
            nig_a = (nig[first], False, False) + tuple(nig[first + 3:first + 3 + na])
            nig_b = (nig[first + 1], False, False) + tuple(nig[first + 3 + na:first + 3 + na + nb])
            programs += rows_mlp.tape_programs(st.tape, dyh[j], dyq[j], nig_a, nig_b, b_leads=j + 1 < n)
        outs = rows_mlp._lockstep(*programs)
        for j, (st, _, first) in enumerate(live):
            oa, ob = outs[2 * j], outs[2 * j + 1]
            grads[first], grads[first + 1], grads[first + 2] = oa[0], ob[0], dbq[j]
            grads[first + 3:first + 3 + len(st.tape.params_a) + len(st.tape.params_b)] = tuple(oa[3:]) + tuple(ob[3:])
        ctx.group = None
        return tuple(grads)


class HeadsForward:
    """What ONE forward pass of the model decides and keeps for its heads: the sink of the base positions' gradient, and the
    group of stages whose backward runs as one node.  `begin(...)`; `.feature` replaces the cluster features (the sink's alias
    where there is one); `.stage(...)` per stage, `.finish(end_points)` behind the last one."""

    def __init__(self, cluster_xyz, cluster_feature, stages, training):
        self.sink, self.group, self.feature = None, None, cluster_feature
        grad = torch.is_grad_enabled()
        if _PAIR_DECODE and _FUSED_DECODE and _XYZ_SINK and cluster_xyz.is_cuda and grad and \
                cluster_xyz.requires_grad and cluster_feature.requires_grad:
            # every stage decodes against cluster_xyz: its seven gradients are summed by the decode kernels themselves
            self.sink = XyzGradSink()
            self.feature = SinkFlush.apply(cluster_feature, cluster_xyz, self.sink)
        if heads_bwd_route(stages, _PAIR_STACKS, _PAIR_DECODE, _FUSED_DECODE, self.feature.is_cuda, training, grad,
                           sa_fused._world(), sa_fused._FORCE_COLLECTIVES) == "group":
            self.group = HeadsGroup()              # the heads' backward of all stages: one node, grouped launches

    def stage(self, head, quad_head, net, net_q, base_xyz, base_xyz_q, end_points, prefix, rows=None, rows_q=None,
              want_pos=False):
        """predict_pair with this forward's sink and group"""
        return predict_pair(head, quad_head, net, net_q, base_xyz, base_xyz_q, end_points, prefix, rows, rows_q,
                            sink=self.sink, want_pos=want_pos, group=self.group)

    def finish(self, end_points):
        if self.group is not None:
            self.group.finish(end_points)


begin = HeadsForward


# ---- the modules ------------------------------------------------------------------------------------------------------------
def decode_scores(base_xyz, objectness_scores, center, heading_scores, heading_residuals_normalized,
                  size_scores, size_residuals_normalized, sem_cls_scores, end_points, num_class,
                  num_heading_bin, num_size_cluster, mean_size_arr, prefix):
    """Store the raw head outputs under `prefix` and decode the predicted box size
    (reference :35-59; the mean-size table follows the scores' device instead of `.cuda()`)."""
    B, K = objectness_scores.shape[0], objectness_scores.shape[1]
    size_residuals_normalized = size_residuals_normalized.view([B, K, num_size_cluster, 3])
    if not torch.is_tensor(mean_size_arr):
        mean_size_arr = torch.from_numpy(np.asarray(mean_size_arr).astype(np.float32))
    means = mean_size_arr.to(size_scores.device).unsqueeze(0).unsqueeze(0)
    size_residuals = size_residuals_normalized * means
    size_recover = size_residuals + means
    pick = torch.argmax(size_scores, -1).unsqueeze(-1).unsqueeze(-1).repeat(1, 1, 1, 3)
    pred_size = torch.gather(size_recover, 2, pick).squeeze(2)
    _publish(HEAD_OUTS, (objectness_scores, center, heading_scores, heading_residuals_normalized,
                         heading_residuals_normalized * (np.pi / num_heading_bin), size_scores, size_residuals_normalized,
                         size_residuals, pred_size, sem_cls_scores), end_points, prefix)
    return end_points, pred_size


def _fused_rows(y):
    """rows as the row kernels leave them (on a GPU, the step's element type, unit stride): the fused decode takes them"""
    return _FUSED_DECODE and y.is_cuda and y.dtype == E16.dtype and y.stride(1) == 1


class _SeatedHeads:
    """What the two prediction heads share: their forward (stack, then the head's own `finish`), and
    copy.deepcopy of a prediction head (the EMA teacher is a deepcopy of the student): Parameter.__deepcopy__ clones every
    parameter into storage of its own, so the copy's output heads are seated into fresh joint buffers right away instead of
    inside its first forward."""

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k != "_omnipq_joint":
                new.__dict__[k] = copy.deepcopy(v, memo)
        with torch.no_grad():
            seat_head_parameters(new)
        return new

    def forward(self, net, base_xyz, end_points, prefix, net_rows=None, problem=None):
        y = head_stack(self, net, self.heads(), net_rows, raw=True, problem=problem)
        return self.finish(y, net, base_xyz, end_points, prefix)


class PredictHead(_SeatedHeads, nn.Module):
    """Object head: 2 x (Conv1d+BN+ReLU) trunk, then seven 1x1 heads (reference :62-91)."""

    def __init__(self, hidden_dim, num_heading_bin, num_size_cluster, num_class, mean_size_arr):
        super().__init__()
        self.num_class = num_class
        self.num_size_cluster = num_size_cluster
        self.mean_size_arr = mean_size_arr
        self.num_heading_bin = num_heading_bin
        self.objectness_scores_head = nn.Conv1d(hidden_dim, 2, 1)
        self.center_head = nn.Conv1d(hidden_dim, 3, 1)
        self.heading_class_head = nn.Conv1d(hidden_dim, num_heading_bin, 1)
        self.heading_residual_head = nn.Conv1d(hidden_dim, num_heading_bin, 1)
        self.size_class_head = nn.Conv1d(hidden_dim, num_size_cluster, 1)
        self.size_residual_head = nn.Conv1d(hidden_dim, num_size_cluster * 3, 1)
        self.sem_cls_scores_head = nn.Conv1d(hidden_dim, num_class, 1)
        self.conv1 = nn.Conv1d(hidden_dim, hidden_dim, 1)
        self.conv2 = nn.Conv1d(hidden_dim, hidden_dim, 1)
        self.bn1 = nn.BatchNorm1d(hidden_dim)
        self.bn2 = nn.BatchNorm1d(hidden_dim)
        self._means = None

    def _mean_sizes(self, device):
        if self._means is None or self._means.device != device:
            self._means = torch.from_numpy(np.asarray(self.mean_size_arr).astype(np.float32)).to(device)
        return self._means

    def heads(self):
        return (self.objectness_scores_head, self.center_head, self.heading_class_head,
                self.heading_residual_head, self.size_class_head, self.size_residual_head,
                self.sem_cls_scores_head)

    def finish(self, y, net, base_xyz, end_points, prefix):
        """From the joint output rows `y` of the seven heads to the `end_points` entries."""
        B, K = net.shape[0], net.shape[2]
        if _fused_rows(y):
            means = self._mean_sizes(net.device)
            outs = HeadDecode.apply(y, base_xyz, means, self.num_heading_bin, self.num_size_cluster, self.num_class)
            _publish(HEAD_OUTS, outs, end_points, prefix)
            return outs[1], outs[8], end_points
        widths = [h.out_channels for h in self.heads()]
        obj, ctr, hcls, hres, scls, sres, sem = torch.split(y[:, :sum(widths)].reshape(B, K, -1), widths, dim=2)
        center = ctr + base_xyz
        end_points, pred_size = decode_scores(
            base_xyz, obj, center, hcls, hres, scls, sres, sem, end_points, self.num_class,
            self.num_heading_bin, self.num_size_cluster, self._mean_sizes(net.device), prefix)
        return center, pred_size, end_points


class QuadPredictHead(_SeatedHeads, nn.Module):
    """Layout-quad head: scores, centre, normal, size (reference :94-121).  The normal is divided
    by the 2-norm of the WHOLE (B,K,3) tensor (:112-113) -- batch-coupled, reproduced as is."""

    def __init__(self, hidden_dim):
        super().__init__()
        self.quad_scores_head = nn.Conv1d(hidden_dim, 2, 1)
        self.center_head = nn.Conv1d(hidden_dim, 3, 1)
        self.normal_vector_head = nn.Conv1d(hidden_dim, 3, 1)
        self.size_head = nn.Conv1d(hidden_dim, 2, 1)
        self.conv1 = nn.Conv1d(hidden_dim, hidden_dim, 1)
        self.conv2 = nn.Conv1d(hidden_dim, hidden_dim, 1)
        self.bn1 = nn.BatchNorm1d(hidden_dim)
        self.bn2 = nn.BatchNorm1d(hidden_dim)

    def heads(self):
        return (self.quad_scores_head, self.center_head, self.normal_vector_head, self.size_head)

    def finish(self, y, net, base_xyz, end_points, prefix):
        B, K = net.shape[0], net.shape[2]
        if _fused_rows(y):
            outs = QuadDecode.apply(y, base_xyz)
        else:
            scores, ctr, normal, size = torch.split(y[:, :10].reshape(B, K, -1), [h.out_channels for h in self.heads()], dim=2)
            outs = (scores, ctr + base_xyz, normal.div(torch.norm(normal, p=2)), size)
        _publish(QUAD_OUTS, outs, end_points, prefix)
        return outs[1], outs[3], end_points
