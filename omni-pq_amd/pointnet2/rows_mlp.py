"""Per-point MLPs on row-major activations, on the same hand-written HIP kernels as the fused SA stage.

The reference applies its small per-point networks as stacks of kernel-size-1 convolutions with
BatchNorm and ReLU on (B, C, K) tensors:
    heads        Conv1d+BN+ReLU x2, then 4-7 output Conv1d        models/pq_transformer.py:62-121
    pos. embed   Conv1d(3->288)+BN+ReLU, Conv1d(288->288)          models/pq_transformer.py:17-33
    voting       Conv1d+BN+ReLU x2, Conv1d(288->291)               models/voting_module.py:32-53
    FP layers    SharedMLP: Conv2d(1x1, no bias)+BN+ReLU x2        pointnet2/pointnet2_modules.py:356-416
Here each stack is ONE autograd node over rows (points x channels, bf16): per layer a MFMA GEMM
(`omnipq_gemm_nt_e16[_bias]`), for BatchNorm layers the statistic / finalize / normalise+ReLU kernels of
csrc/sa_stage.hip, and in backward the matching `bn_bwd_*` kernels, the data-gradient GEMM and the
split-K weight-gradient GEMM.  Training-mode BatchNorm semantics are the reference's (batch statistics,
momentum update of the running estimates, SyncBatchNorm all-reduce of the sums under a process group).  A
linear bias that feeds a BatchNorm is never added: the batch mean removes it again; only the running
mean accounts for it (and its gradient is exactly zero).

Used under `torch.autocast("cuda", dtype=torch.bfloat16)` (or float16: sa_fused.E16); otherwise callers keep PyTorch's f32 layers.
"""
import collections
import ctypes
import functools
import os
import typing

import torch

import dropout_state
import sa_fused
from sa_fused import E16, _call, _gemm_nt_bnbwd, _gemm_nt_stats, _gemm_tn, _lib, _p, _round_up, _world, prep_weight, unprep_wgrad, zeros_f32

# ReLU + dropout of a `relu_dropout` layer inside its GEMM's epilogue, and its backward mask in the epilogue of the data-gradient
# GEMM above it (False: the separate in-place passes; tests/test_gpu_decoder.py:
# test_rows_stack_with_and_without_fused_activation compares the two)
_FUSE_ACT = True


class Layer:
    """One linear layer of the stack: weight (C_out, C_in[,1[,1]]), optional bias, optional BatchNorm
    module (BatchNorm1d/2d/SyncBatchNorm; with it a ReLU follows, as everywhere in the reference), or --
    without BatchNorm -- `relu_dropout=p`: ReLU then dropout(p) on the output (the decoder's feed-forward,
    transformer.py:222; p = 0 in eval mode)."""

    def __init__(self, weight, bias=None, bn=None, relu_dropout=None):
        self.weight, self.bias, self.bn, self.relu_dropout = weight, bias, bn, relu_dropout


def enabled():
    """OMNIPQ_ROWS=torch keeps every per-point MLP on PyTorch's own kernels (A/B runs and the parity tests that put
    torch's bf16 autocast next to the hand-written path)."""
    return os.environ.get("OMNIPQ_ROWS", "rows") != "torch"


def usable(x, layers, training):
    """bf16 autocast on a GPU, training-mode BN (or no grad in eval), widths the kernels accept."""
    if not enabled():
        return False
    if not x.is_cuda or not E16.autocast():
        return False
    for lay in layers:
        if lay.bn is not None:
            bn = lay.bn
            if bn.weight is None or bn.running_mean is None or bn.momentum is None:
                return False
            if lay.weight.shape[0] % 32 or lay.weight.shape[0] > 640:      # kernel limits (multiples of the K step)
                return False
            if not training and torch.is_grad_enabled():
                return False
            if sa_fused.bn_syncs(bn) is None:            # SyncBatchNorm on a custom process group: torch's own path
                return False
    return True


def run(x_rows, layers, training, padded=False, eval_chain=False):
    """x_rows (N, C_in) -> (N, C_out of the last layer), bf16.  padded: return the kernels' own (N, C_out rounded
    up to 32) buffer instead of the slice -- the extra columns are exact zeros (zero weight rows and bias), and a
    consumer that hands back a gradient of that shape saves the stack a zero-fill and a copy.  eval_chain: the caller opts
    into the one-launch inference route (see EVAL_CHAIN) for the calls stack_route sends there; every other call is run as
    without the keyword."""
    if eval_chain:
        route = _chain_route(x_rows, layers, training)
        if route is not None:
            return _infer(x_rows, layers, route, padded)
    spec, params = _spec_of(x_rows, layers, training, padded)
    return RowsMLP.apply(x_rows, spec, bool(training), *params)


# What follows a layer's linear map (run / run_pair pass these to the autograd nodes as non-tensor arguments; None: nothing).
# BnSpec: BatchNorm + ReLU, the module's buffers and constants.  ActSpec: ReLU + dropout(p), seed and salt pick the mask
# (dropout_state; p = 0: no seed).  StackSpec: layers = one of them per layer, padded: see run(), sync: the BatchNorm layers are
# SyncBatchNorm (statistics over all ranks).
BnSpec = collections.namedtuple("BnSpec", "running_mean running_var num_batches_tracked momentum eps")
ActSpec = collections.namedtuple("ActSpec", "p seed salt")
StackSpec = collections.namedtuple("StackSpec", "layers padded sync")


def _kind(spec):
    return "bn" if isinstance(spec, BnSpec) else "act" if isinstance(spec, ActSpec) else "plain"


class LayerRoute(typing.NamedTuple):
    kind: str         # "bn" | "act" | "plain"
    feed: str         # the GEMM's operand: "input" (layer 0: the prepared input rows) | "stored" (the layer below's output) | "yab"
                      # (rebuilt from the layer below's pre-BN output and its scale / shift while the GEMM stages it) | "lds" (chain:
                      # the layer below's output, which never leaves the workgroup)
    gemm: str         # "stats" (with the batch statistics of its output) | "relu_dropout" (ReLU + dropout in its epilogue) | "plain";
                      # on a "yab" feed the affine entry point of the same kind | "chain" (every layer of the stack: ONE forward-only
                      # launch, omnipq_rows_infer; the backward fields are "")
    finalize: str     # bn: where the layer's constants are derived: "consumer" (the prologue of the GEMM it feeds, nothing stored) |
                      # "launch" (omnipq_bn_finalize_relu) | "running" (eval: from the running estimates, + omnipq_bnrelu) | "folded"
                      # (chain: from the running estimates inside the launch); else ""
    act: str          # act: ReLU + dropout in the GEMM's "epilogue" | the in-place "pass" (omnipq_relu_dropout); else ""
    dgrad: str        # the data gradient: "input" (layer 0: only if the input needs one) | "bnbwd" (with the BatchNorm-backward totals
                      # of the layer below) | "mask" (with the layer below's ReLU + dropout mask in its epilogue) | "plain"
    bwd_stats: str    # bn: its BatchNorm-backward totals come from the data-gradient GEMM "above" | its "own" launch; else ""
    bwd_act: str      # act: its backward mask is applied by the data-gradient GEMM "above" | its own "pass"; else ""


class StackRoute(typing.NamedTuple):
    """Every decision of one stack pass, made by stack_route() before anything is launched.  _forward_program stores it on its
    context; forward and backward dispatch on it and decide nothing themselves.  A new route is a new value of a field of
    LayerRoute, its condition in stack_route(), and a step function for the two programs to call.  (What depends on the moment
    of the launch stays there: the statistics exchange, deferred weight gradients, the input cache, PairStats.)"""
    training: bool
    layers: tuple     # one LayerRoute per layer


# The INFERENCE stack in one launch (csrc/rows_infer.hip, include/omnipq_decoder.h: omnipq_rows_infer).  In eval
# mode BatchNorm is the affine a = gamma / sqrt(running_var + eps), b = beta - (running_mean - bias) a, known before the launch:
# a tile of rows goes from the input to the last layer's output inside one workgroup, every hidden activation rounded once and
# never stored.  Taken when nothing can ask for a backward -- eval mode, the call made under torch.no_grad() -- and only where
# the caller opted in (run / run_pair: eval_chain=True).  EVAL_CHAIN = False restores the stored dataflow (one GEMM, the
# rebuilt constants and omnipq_bnrelu per layer) everywhere.
EVAL_CHAIN = True
eval_chain_uses = 0
_InferLayer = sa_fused._ext.rows_infer_layer_struct()


@functools.lru_cache(maxsize=None)
def _infer_lds_bytes(kpad, widths):
    return int(_lib.omnipq_rows_infer_lds_bytes(kpad, len(widths), (ctypes.c_int * max(len(widths), 1))(*widths)))


def eval_chain_ok(cin, widths):
    """the shapes omnipq_rows_infer takes (one to three layers of 32 k <= 640 channels, an input of at most 1024 channels and an
    LDS footprint the CU has): asked of the library, which refuses exactly the others.  widths: as the kernels hold them
    (rounded up to 32, what omnipq_prep_weight leaves)."""
    return cin > 0 and _infer_lds_bytes(_round_up(int(cin), 32), tuple(int(w) for w in widths)) > 0


def stack_route(training, N, cin, layers, no_grad=False):
    """The route of a stack from shapes alone (no tensor, no launch; the switches are read now).  N rows of cin channels;
    layers: per layer (output channels, kind).  no_grad: the call is made under torch.no_grad() (read by the caller, outside
    any autograd Function: inside Function.forward grad mode is always off) -- an eval stack with a hidden layer whose shape
    the library takes is then ONE launch: gemm "chain", operands from the "input" / from "lds", BatchNorm "folded"."""
    if no_grad and not training and EVAL_CHAIN and len(layers) >= 2 and \
            all(cout % 32 == 0 for cout, kind in layers if kind == "bn") and \
            eval_chain_ok(cin, tuple(_round_up(cout, 32) for cout, _ in layers)):
        return StackRoute(False, tuple(LayerRoute(kind, "lds" if l else "input", "chain", "folded" if kind == "bn" else "",
                                                  "epilogue" if kind == "act" else "", "", "", "")
                                       for l, (_, kind) in enumerate(layers)))
    L, K, out = len(layers), _round_up(cin, 32), []
    for l, (cout, kind) in enumerate(layers):
        Cp = _round_up(cout, 32)
        feed = "input" if l == 0 else "yab" if out[-1].finalize == "consumer" else "stored"
        if kind == "bn" and training:
            gemm = "stats"
        elif kind == "act" and feed != "yab" and _FUSE_ACT and K < 1024 and N * Cp < (1 << 32):
            gemm = "relu_dropout"             # (the widths the epilogue kernel is built for; its mask hashes a 32-bit element index)
        else:
            gemm = "plain"
        finalize = ""
        if kind == "bn":
            # "consumer": relu(bn(Y)) is never stored: the next layer's GEMM and this layer's consumers in backward rebuild it
            # from (Y, a, b) while staging their operand, and the finalize happens in the prologue of that GEMM
            finalize = "running" if not training else \
                "consumer" if (l < L - 1 and sa_fused.affine_pays(N, layers[l + 1][0])) else "launch"
        below = layers[l - 1][1] if l else None
        dgrad = "input" if l == 0 else "bnbwd" if below == "bn" else \
            "mask" if (below == "act" and _FUSE_ACT and Cp < 1024) else "plain"
        out.append(LayerRoute(kind, feed, gemm, finalize, "" if kind != "act" else "epilogue" if gemm == "relu_dropout" else "pass",
                              dgrad, "" if kind != "bn" else "above" if l < L - 1 else "own", ""))
        K = Cp
    for l, r in enumerate(out):
        if r.kind == "act":
            out[l] = r._replace(bwd_act="above" if (l < L - 1 and out[l + 1].dgrad == "mask") else "pass")
    return StackRoute(bool(training), tuple(out))


class _L:
    """Per-layer constants and saved tensors (the attributes sa_fused's helpers read of a layer: Y, a, b, mean, invstd, fin)."""
    __slots__ = ("act", "K", "C", "Cp", "Wp", "Wt", "wk", "a", "b", "mean", "invstd", "Y", "X", "has_bias", "fin")


def _hold(lead):
    """Before a GEMM of the LEADING stack of a pair: the launch is held back for its partner's (csrc: omnipq_pair_hold)."""
    if lead:
        _lib.omnipq_pair_hold()


def _drain(gen):
    """Run one stack's program on its own."""
    assert not _lib.omnipq_pair_held(), "rows_mlp: a held pair launch leaked into a lone stack"
    try:
        while True:
            next(gen)
    except StopIteration as done:
        return done.value


def _lockstep(*gens):
    """Run independent stacks' programs GEMM by GEMM: each program stops right after issuing a GEMM; the leading ones' (all but
    the last program) are held back and go out in one grid with the last program's next GEMM of the same kind (held launches
    that find no partner are sent out before anything else can be enqueued behind them).  Two programs pair (omnipq_pair_hold);
    more open a group per round (omnipq_pair_group: no statistics exchange is shared, the caller runs such a group only
    where none is needed)."""
    n = len(gens)
    out = [None] * n
    alive = [True] * n
    assert not _lib.omnipq_pair_held(), "rows_mlp: a pair launch was still held when a lockstep run started"
    outer, sa_fused.PairStats.active = sa_fused.PairStats.active, sa_fused.PairStats() if n == 2 else None
    try:
        while any(alive):
            if n > 2:
                _lib.omnipq_pair_group(sum(alive))
            for i in range(n):
                if not alive[i]:
                    continue
                held = _lib.omnipq_pair_held()
                try:
                    next(gens[i])
                except StopIteration as done:
                    out[i], alive[i] = done.value, False
                if i < n - 1 and _lib.omnipq_pair_held() != held + 1:
                    _lib.omnipq_pair_flush()              # nothing was held: disarm before the next program runs
            _lib.omnipq_pair_flush()
    finally:
        sa_fused.PairStats.active = outer
        _lib.omnipq_pair_flush()      # an exception in a program must not leave a launch held or the hold armed
    assert not _lib.omnipq_pair_held()
    return out


class _Ctx:
    """What a stack's program keeps between forward and backward (one per stack of a pair; a lone stack uses the autograd
    context itself)."""
    __slots__ = ("route", "layers", "X0", "geom", "wshapes", "nbias", "targets", "in_dtype", "padded")


# ---- forward steps ----

def _input_rows(x, N, cin, K):
    """x (N, cin) -> the first GEMM's operand: E16 rows (N, K), zero-padded.  The same input tensor feeding several stacks (the
    decoder's key positions: one embedding per layer) is prepared once; the copy is tied to the tensor's version counter, so
    an input updated in place (a static buffer refilled with copy_) is converted again instead of feeding stale rows."""
    cached = getattr(x, "omnipq_rows_in", None)
    if cached is not None and cached[0] == x._version and cached[1].shape == (N, K):
        return cached[1]
    if K == cin:
        X = x.detach().to(E16.dtype).contiguous()
    elif x.dtype in (torch.float32, E16.dtype) and x.stride(1) == 1:
        X = torch.empty((N, K), device=x.device, dtype=E16.dtype)          # cast + zero padding in one launch
        _call(_lib.omnipq_pad_rows_e16, x, N, cin, K, x.stride(0), _p(x), int(x.dtype == torch.float32), _p(X))
    else:
        X = torch.nn.functional.pad(x.detach().to(E16.dtype), (0, K - cin))
    if X.data_ptr() != x.data_ptr() and not x.requires_grad:
        try:
            x.omnipq_rows_in = (x._version, X)    # inputs without gradient only: constants of the forward pass
        except Exception:
            pass
    return X


def _new_layer(W, bias, K, act, training):
    """The layer's sizes and its prepared weight; act: its ActSpec, if it has one."""
    lay = _L()
    W2 = W.detach().reshape(W.shape[0], -1)
    lay.C, lay.wk = W2.shape
    lay.K, lay.Cp = K, _round_up(lay.C, 32)
    lay.has_bias, lay.act, lay.fin = bias is not None, act, None
    lay.Wp, lay.Wt = prep_weight(W2, lay.Cp, K, transpose=training, persistent=sa_fused.is_persistent(W))
    return lay


def _padded_bias(bias, Cp):
    bp = bias.detach().float()                 # may come zero-padded already (cat_params(pad_to=))
    return bp if bp.shape[0] >= Cp else torch.nn.functional.pad(bp, (0, Cp - bp.shape[0]))


# the forward GEMM of a layer, by LayerRoute.gemm: (lay, X, below, N, bias, sums) -> Y.  below: the layer X is rebuilt from
# (feed "yab"; X is None then)
def _gemm_stats(lay, X, below, N, bias, sums):
    if below is not None:
        return sa_fused.gemm_nt_affine(below.Y, below, lay.Wp, N, lay.Cp, lay.K, sums=sums)
    return _gemm_nt_stats(X, lay.Wp, N, lay.Cp, lay.K, sums)


def _gemm_relu_dropout(lay, X, below, N, bias, sums):
    """ReLU + dropout in the GEMM's epilogue (same decisions as omnipq_relu_dropout on the stored matrix)"""
    Y = torch.empty((N, lay.Cp), device=X.device, dtype=E16.dtype)
    _call(_lib.omnipq_gemm_nt_e16_relu_dropout, X, N, lay.Cp, lay.K, _p(X), lay.K, _p(lay.Wp), lay.K, _p(Y), lay.Cp, _p(bias),
          lay.act.p, _p(lay.act.seed), lay.act.salt)
    return Y


def _gemm_plain(lay, X, below, N, bias, sums):
    Y = torch.empty((N, lay.Cp), device=lay.Wp.device, dtype=E16.dtype)
    if below is not None:
        sa_fused.gemm_nt_affine(below.Y, below, lay.Wp, N, lay.Cp, lay.K, bias=bias, out=Y)
    else:
        sa_fused.gemm_nt_into(X, lay.Wp, Y, N, lay.Cp, lay.K, bias=bias)
    return Y


_GEMM = {"stats": _gemm_stats, "relu_dropout": _gemm_relu_dropout, "plain": _gemm_plain}


# where a BatchNorm layer gets its constants, by LayerRoute.finalize: (lay, N, count, sums, bn, bias, gamma, beta) -> lay.X
def _finalize_in_consumer(lay, N, count, sums, bn, bias, gamma, beta):
    """by the GEMM this layer feeds (sa_fused.gemm_nt_affine takes `fin`); relu(bn(Y)) is never stored"""
    lay.fin = sa_fused.batch_constants(lay, sums, count, gamma, beta, bn, bias)
    lay.X = None
    return None


def _finalize_launch(lay, N, count, sums, bn, bias, gamma, beta):
    return sa_fused.finalize_launch(lay, N, sa_fused.batch_constants(lay, sums, count, gamma, beta, bn, bias), relu=True)


def _finalize_running(lay, N, count, sums, bn, bias, gamma, beta):
    """eval mode: constants from the running estimates, then normalise + ReLU"""
    return sa_fused.running_constants(lay, N, gamma, beta, bn, bias)


_FINALIZE = {"consumer": _finalize_in_consumer, "launch": _finalize_launch, "running": _finalize_running}


def _forward_program(ctx, lead, x, spec, training, params):
    dev = x.device
    N, cin = x.shape
    L = len(spec.layers)
    world = _world() if (training and spec.sync) else 1
    route = stack_route(training, N, cin, tuple((params[4 * l].shape[0], _kind(spec.layers[l])) for l in range(L)))
    X0 = X = _input_rows(x, N, cin, _round_up(cin, 32))
    K = X.shape[1]
    layers = []
    for l, r in enumerate(route.layers):
        W, bias, gamma, beta = params[4 * l:4 * l + 4]
        lay = _new_layer(W, bias, K, spec.layers[l] if r.kind == "act" else None, training)
        if r.kind == "bn" and lay.Cp != lay.C:
            raise RuntimeError("RowsMLP: BatchNorm widths must be multiples of 32")
        sums, slot = sa_fused.pair_sums(lead, 2, lay.C, dev, world) if r.gemm == "stats" else (None, None)
        # (a linear bias that feeds a BatchNorm is never added: see the module's docstring)
        bp = _padded_bias(bias, lay.Cp) if (lay.has_bias and r.kind != "bn") else None
        _hold(lead)
        lay.Y = _GEMM[r.gemm](lay, X, layers[-1] if r.feed == "yab" else None, N, bp, sums)
        yield
        if r.kind == "bn":
            if training:
                sa_fused.pair_allreduce(sums, slot, lead, world)
            X = _FINALIZE[r.finalize](lay, N, float(N) * world, sums, spec.layers[l], bias, gamma, beta)
            if training:
                sa_fused.bump(spec.layers[l].num_batches_tracked)
        else:
            if r.act == "pass":
                _call(_lib.omnipq_relu_dropout, lay.Y, N * lay.Cp, _p(lay.Y), lay.act.p, _p(lay.act.seed), lay.act.salt)
            X = lay.X = lay.Y
        K = lay.Cp
        layers.append(lay)
    ctx.route, ctx.layers, ctx.X0, ctx.geom = route, layers, X0, (N, cin, world)
    ctx.wshapes = [tuple(params[4 * l].shape) for l in range(L)]
    ctx.nbias = [0 if params[4 * l + 1] is None else params[4 * l + 1].shape[0] for l in range(L)]
    # where the weight / bias gradients may be written directly (sa_fused.deferred_wgrads)
    ctx.targets = [(sa_fused.grad_target(params[4 * l]),
                    None if params[4 * l + 1] is None else sa_fused.grad_target(params[4 * l + 1]))
                   for l in range(L)] if training else None
    ctx.in_dtype, ctx.padded = x.dtype, spec.padded
    last = layers[-1]
    return X if (spec.padded or last.Cp == last.C) else X[:, :last.C]


# ---- the inference chain (route "chain": see EVAL_CHAIN) ----

def _layer_kind(lay):
    return "bn" if lay.bn is not None else "act" if lay.relu_dropout is not None else "plain"


def _chain_route(x, layers, training):
    """the stack's route if stack_route sends this call to the chain, else None.  Grad mode is read HERE."""
    if training or torch.is_grad_enabled() or x.dim() != 2:
        return None
    route = stack_route(False, x.shape[0], x.shape[1], tuple((lay.weight.shape[0], _layer_kind(lay)) for lay in layers), no_grad=True)
    return route if route.layers[0].gemm == "chain" else None


def _infer(x, layers, route, padded):
    """the whole stack as ONE launch (omnipq_rows_infer) -> (N, C_out) E16, or the kernel's own (N, C_out rounded up to 32)
    buffer with padded"""
    global eval_chain_uses
    N, cin = x.shape
    x = x.detach()
    if x.dtype not in (torch.float32, E16.dtype) or x.stride(1) != 1:
        x = x.to(E16.dtype).contiguous()
    L = len(layers)
    recs = (_InferLayer * L)()
    keep = []                                   # what the records point to
    K = _round_up(cin, 32)
    for lay, r, rec in zip(layers, route.layers, recs):
        nl = _new_layer(lay.weight, lay.bias, K, None, False)
        if r.kind == "bn":
            bn = lay.bn
            vecs = [v.detach().float().contiguous() for v in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
            rec.gamma, rec.beta, rec.running_mean, rec.running_var = (v.data_ptr() for v in vecs)
            rec.eps = float(bn.eps)
            bias = None if lay.bias is None else lay.bias.detach().float().contiguous()
        else:
            vecs = []
            # (no copy where the bias arrives f32 and padded, as the heads' joint bias does; a narrower one is padded per call,
            # as on the stored route: a copy kept across calls would miss an optimizer that writes the parameter by pointer)
            bias = None if lay.bias is None else _padded_bias(lay.bias, nl.Cp).contiguous()
        rec.W, rec.ldw, rec.C = nl.Wp.data_ptr(), nl.Wp.stride(0), nl.Cp
        rec.bias = 0 if bias is None else bias.data_ptr()
        rec.relu = int(r.kind != "plain")
        keep.append((nl.Wp, bias, vecs))
        K = nl.Cp
    Y = torch.empty((N, K), device=x.device, dtype=E16.dtype)
    _call(_lib.omnipq_rows_infer, Y, N, cin, x.stride(0) if N > 1 else cin, _p(x), int(x.dtype == torch.float32), L,
          ctypes.c_void_p(ctypes.addressof(recs)), _p(Y))
    eval_chain_uses += 1
    C = layers[-1].weight.shape[0]
    return Y if (padded or K == C) else Y[:, :C]


# ---- backward steps ----

def _output_grad(g, last, N, padded):
    """-> (the gradient as E16 rows of the last layer's padded width, whether the buffer is this program's to overwrite)"""
    if last.Cp == last.C or padded:
        dcur = g.to(E16.dtype).contiguous()
        return dcur, dcur.data_ptr() != g.data_ptr()        # autograd's buffer must not be modified in place
    dcur = torch.zeros((N, last.Cp), device=g.device, dtype=E16.dtype)
    dcur[:, :last.C] = g
    return dcur, True


def _bn_bwd_stats(lay, dcur, N, sums):
    """the BatchNorm-backward totals of a layer that no data-gradient GEMM above it produced (LayerRoute.bwd_stats "own")"""
    _call(_lib.omnipq_bn_bwd_stats_z, dcur, N, lay.C, _p(dcur), _p(lay.Y), _p(lay.a), _p(lay.b), _p(lay.mean), _p(lay.invstd),
          _p(sums))


def _act_bwd(lay, dcur, dst, N):
    """lay.Y holds dropout(relu(.)): positive exactly where the unit was active and kept"""
    _call(_lib.omnipq_relu_dropout_bwd, dcur, N * lay.Cp, _p(lay.Y), _p(dcur), _p(dst), lay.act.p)


def _weight_grad(ctx, l, dcur, Xin, below, dfr, needs_input_grad, grads):
    """dW (and the bias gradient: column sums of dY, from the same pass) of layer l, now or -- inside deferred_wgrads, where
    the parameters can be written directly -- with all the others when the block ends"""
    lay, N = ctx.layers[l], ctx.geom[0]
    want_bias = ctx.route.layers[l].kind != "bn" and lay.has_bias
    wt, bt = ctx.targets[l] if (dfr is not None and ctx.targets is not None) else (None, None)
    if wt is not None and needs_input_grad[3 + 4 * l] and (
            not want_bias or (sa_fused.bias_target_ok(bt, lay.C, lay.Cp) and needs_input_grad[4 + 4 * l])):
        dfr.add(dcur, Xin, lay.Cp, lay.K, N, wt, sa_fused.Crop(lay.C, lay.wk), bt if want_bias else None, below)
        return
    bsum = None
    if want_bias:
        bsum = zeros_f32(lay.Cp, dcur.device)
        grads[4 * l + 1] = bsum[:ctx.nbias[l]]
    dWp = _gemm_tn(dcur, Xin, lay.Cp, lay.K, N, colsum=bsum, below=below)
    grads[4 * l] = unprep_wgrad(dWp, lay.C, lay.wk, 0, ctx.wshapes[l])      # in the parameter's own shape


# the data gradient of a layer, by LayerRoute.dgrad: (lay, under, dcur, N, sums) -> gradient w.r.t. the layer's operand;
# under: the layer below
def _dgrad_bnbwd(lay, under, dcur, N, sums):
    return _gemm_nt_bnbwd(dcur, lay.Wt, N, lay.K, lay.Cp, under, sums)


def _dgrad_mask(lay, under, dcur, N, sums):
    """the layer below is dropout(relu(.)): its backward mask in this GEMM's epilogue"""
    dprev = torch.empty((N, lay.K), device=dcur.device, dtype=E16.dtype)
    _call(_lib.omnipq_gemm_nt_e16_mask, dcur, N, lay.K, lay.Cp, _p(dcur), lay.Cp, _p(lay.Wt), lay.Cp, _p(dprev), lay.K,
          _p(under.Y), under.act.p)
    return dprev


def _dgrad_plain(lay, under, dcur, N, sums):
    dprev = torch.empty((N, lay.K), device=dcur.device, dtype=E16.dtype)
    sa_fused.gemm_nt_into(dcur, lay.Wt, dprev, N, lay.K, lay.Cp)
    return dprev


_DGRAD = {"bnbwd": _dgrad_bnbwd, "mask": _dgrad_mask, "plain": _dgrad_plain, "input": _dgrad_plain}


def _backward_program(ctx, lead, g, needs_input_grad):
    route, layers = ctx.route, ctx.layers
    if not route.training and any(r.kind == "bn" for r in route.layers):
        raise RuntimeError("RowsMLP: backward through eval-mode BatchNorm is not supported")
    N, cin, world = ctx.geom
    L = len(layers)
    dev = g.device
    grads = [None] * (4 * L)
    dcur, owned = _output_grad(g, layers[-1], N, ctx.padded)
    dx = None
    sums = slot = None        # BatchNorm-backward totals that a "bnbwd" data gradient produced for the layer below it, and the
                              # pair buffer they live in (sa_fused.PairStats)
    dfr = sa_fused.deferred_wgrads.active
    for l in range(L - 1, -1, -1):
        lay, r = layers[l], route.layers[l]
        below = layers[l - 1] if r.feed == "yab" else None      # the operand was rebuilt from its pre-BN output inside the GEMM
        Xin = ctx.X0 if r.feed == "input" else layers[l - 1].Y if r.feed == "yab" else layers[l - 1].X
        if r.kind == "bn":
            if r.bwd_stats == "own":
                sums, slot = sa_fused.pair_sums(lead, 3, lay.C, dev, world)
                _bn_bwd_stats(lay, dcur, N, sums)
                if sa_fused.PairStats.active is not None and (world > 1 or sa_fused._FORCE_COLLECTIVES):
                    yield              # the partner's statistics kernel goes out before the exchange both share
            assert sums is not None
            dst = dcur if owned else torch.empty_like(dcur)
            _hold(lead)
            grads[4 * l + 2], grads[4 * l + 3] = sa_fused.bn_backward_apply(dcur, lay, N, lay.C, float(N) * world, sums, world,
                                                                            out=dst, pair=(slot, lead))
            yield
            dcur, owned = dst, True
            if lay.has_bias:
                grads[4 * l + 1] = zeros_f32(lay.C, dev)                # removed by the batch mean
        elif r.bwd_act == "pass":
            dst = dcur if owned else torch.empty_like(dcur)
            _act_bwd(lay, dcur, dst, N)
            dcur, owned = dst, True
        _weight_grad(ctx, l, dcur, Xin, below, dfr, needs_input_grad, grads)
        sums = slot = None
        if r.dgrad == "input" and not needs_input_grad[0]:
            break
        if r.dgrad == "bnbwd":
            sums, slot = sa_fused.pair_sums(lead, 3, lay.K, dev, world)
        _hold(lead)
        dprev = _DGRAD[r.dgrad](lay, layers[l - 1] if l else None, dcur, N, sums)
        yield
        if l > 0:
            dcur, owned = dprev, True
        else:
            dx = dprev[:, :cin].to(ctx.in_dtype)
    ctx.layers = None
    return (dx, None, None, *grads)


class RowsMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, spec, training, *params):
        ctx.e16 = E16.dtype
        return _drain(_forward_program(ctx, False, x, spec, training, params))

    @staticmethod
    def backward(ctx, g):
        E16.select(ctx.e16)
        return _drain(_backward_program(ctx, False, g, ctx.needs_input_grad))


class RowsMLPPair(torch.autograd.Function):
    """Two independent stacks as one node: (xa, spec_a, xb, spec_b, training, n_a, *params_a, *params_b) -> (ya, yb).  Same
    programs as `RowsMLP`, run in lockstep so that the stacks' GEMMs of the same kind share a launch (`_lockstep`)."""

    @staticmethod
    def forward(ctx, xa, spec_a, xb, spec_b, training, n_a, *params):
        ctx.e16 = E16.dtype
        ctx.a, ctx.b, ctx.n_a = _Ctx(), _Ctx(), n_a
        ctx.set_materialize_grads(False)            # a stack unused downstream gets None, not a zero gradient to push through
        ya, yb = _lockstep(_forward_program(ctx.a, True, xa, spec_a, training, params[:n_a]),
                           _forward_program(ctx.b, False, xb, spec_b, training, params[n_a:]))
        return ya, yb

    @staticmethod
    def backward(ctx, ga, gb):
        E16.select(ctx.e16)
        nig, n_a = ctx.needs_input_grad, ctx.n_a
        nig_a = (nig[0], False, False) + tuple(nig[6:6 + n_a])
        nig_b = (nig[2], False, False) + tuple(nig[6 + n_a:])
        if ga is None and gb is None:
            return (None,) * len(nig)
        if ga is None or gb is None:                 # one stack unused downstream: nothing to pair
            outs = []
            for c, g, n in ((ctx.a, ga, nig_a), (ctx.b, gb, nig_b)):
                outs.append(_drain(_backward_program(c, False, g, n)) if g is not None else (None,) * len(n))
            oa, ob = outs
        else:
            oa, ob = _lockstep(*tape_programs(ctx, ga, gb, nig_a, nig_b))
        return (oa[0], None, ob[0], None, None, None) + tuple(oa[3:]) + tuple(ob[3:])


def _spec_of(x_rows, layers, training, padded):
    spec, params = [], []
    for lay in layers:
        bn = lay.bn
        if bn is None and lay.relu_dropout is not None:
            p = float(lay.relu_dropout) if training else 0.0
            spec.append(ActSpec(p, dropout_state.seed(x_rows.device) if p > 0 else None, dropout_state.next_salt() if p > 0 else 0))
        else:
            spec.append(None if bn is None else
                        BnSpec(bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.momentum), float(bn.eps)))
        params += [lay.weight, lay.bias, None if bn is None else bn.weight, None if bn is None else bn.bias]
    # SyncBatchNorm semantics (statistics over all ranks) only where the layers ARE SyncBatchNorm; a stack of plain
    # BatchNorm layers keeps per-rank statistics under DDP, as torch's does
    bns = [lay.bn for lay in layers if lay.bn is not None]
    sync = bool(bns) and all(bool(sa_fused.bn_syncs(bn)) for bn in bns)
    return StackSpec(tuple(spec), bool(padded), sync), params


def run_pair(xa, layers_a, xb, layers_b, training, padded=False, eval_chain=False):
    """`run` on two independent stacks (e.g. the object and the quad head of a decoder stage: same shapes, different
    weights) whose GEMMs go out pairwise in one launch each.  -> (ya, yb).  eval_chain: see run(); a pair whose two stacks
    both go to the chain is two chain launches."""
    if eval_chain:
        ra, rb = _chain_route(xa, layers_a, training), _chain_route(xb, layers_b, training)
        if ra is not None and rb is not None:
            return _infer(xa, layers_a, ra, padded), _infer(xb, layers_b, rb, padded)
    spec_a, params_a = _spec_of(xa, layers_a, training, padded)
    spec_b, params_b = _spec_of(xb, layers_b, training, padded)
    return RowsMLPPair.apply(xa, spec_a, xb, spec_b, bool(training), len(params_a), *params_a, *params_b)


class _Taped:
    """Stands in for the autograd context of a Function whose forward is run outside autograd: keeps what it saves."""
    saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def set_materialize_grads(self, value):
        pass

    def mark_non_differentiable(self, *tensors):
        pass


def tape_pair(xa, layers_a, xb, layers_b, training, padded=False):
    """The forward of `run_pair`'s node OUTSIDE autograd, for a caller that runs the backward of several pairs itself (the
    prediction heads of all stages: models/pred_heads.py).  -> (ya, yb, tape); tape.params_a / tape.params_b are the two
    stacks' parameters in the order `tape_programs` reports their gradients."""
    spec_a, params_a = _spec_of(xa, layers_a, training, padded)
    spec_b, params_b = _spec_of(xb, layers_b, training, padded)
    tape = _Taped()
    tape.params_a, tape.params_b = tuple(params_a), tuple(params_b)
    with torch.no_grad():
        ya, yb = RowsMLPPair.forward(tape, xa, spec_a, xb, spec_b, bool(training), len(params_a), *params_a, *params_b)
    return ya, yb, tape


def tape_programs(tape, ga, gb, nig_a, nig_b, b_leads=False):
    """-> the two backward programs of a pair (a tape, or the pair node's own context) for `_lockstep`: each returns (dx,
    None, None, *parameter gradients).  nig_a / nig_b: (input, False, False, *parameters) need a gradient; the first program
    always leads, the second where further programs follow it in the same lockstep run."""
    return _backward_program(tape.a, True, ga, nig_a), _backward_program(tape.b, b_leads, gb, nig_b)
