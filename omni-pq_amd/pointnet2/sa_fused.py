"""Fused set-abstraction stage for MI355X: group -> shared MLP (conv1x1 + BatchNorm + ReLU) -> max-pool,
forward and backward, on hand-written HIP kernels (csrc/sa_stage.hip, gemm_bf16.hip, gemm_tn_bf16.hip)
reached through the C ABI in include/omnipq_sa.h.

It replaces, for one `PointnetSAModuleVotes`, the chain the reference runs as separate PyTorch ops
(pointnet2_modules.py:243-257):
    grouped = QueryAndGroup(...)          (B, 3+C, M, S) f32        pointnet2_utils.py:317-376
    y = SharedMLP(grouped)                3 x [Conv2d 1x1, BatchNorm2d, ReLU]   pytorch_utils.py:11-36
    out = max_pool2d(y, [1, S])           (B, C_out, M)
with the same parameters (`mlp_module.layer{i}.conv.weight`, `...bn.bn.{weight,bias,running_*}`), the
same training-mode BatchNorm semantics (batch statistics over all B*M*S positions, biased variance for
normalisation, unbiased for the running estimate, momentum update, SyncBatchNorm all-reduce of the
statistics when a process group is up) and the same gradients.

Numerics: activations are stored in bf16, every contraction accumulates in f32 on the MFMA units,
statistics are f32 per block / f64 across blocks.  This is the `bf16` compute mode of bench.py; the f32
parity mode keeps the reference's op-by-op composition (pointnet2_modules.py).
"""
import collections
import ctypes
import functools
import os
import threading
import typing
import weakref

import torch
import torch.distributed as dist

import pointnet2_utils
import wgrads
from wgrads import Crop, bias_target_ok, cat_params, grad_target, joint_params        # noqa: F401  (re-exported)

_ext = pointnet2_utils._load_ext()      # always the product binding, whatever pointnet2_utils._ext is
_lib = _ext._lib
E16 = _ext.E16                         # the 16-bit element type the hand-written kernels run in (bfloat16 / float16)
if os.environ.get("OMNIPQ_TN_DEBUG"):          # A/B runs only: bit 0 = the register-prefetch program of the weight-gradient kernels
    _lib.omnipq_tn_debug(int(os.environ["OMNIPQ_TN_DEBUG"]))


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _call(fn, anchor, *args):
    # plan-aware entry points (include/omnipq_sa.h: `const omnipq_row_plan *plan` before the stream) get the plan of the
    # enclosing `with _row_plan(...)` block of THIS Python thread -- an argument of the call, no state inside the library
    if fn.__name__ in PLAN_AWARE:
        _ext._run(fn, anchor, *args, _plan_state.arg)
    else:
        _ext._run(fn, anchor, *args)


# asked of the loaded library (omnipq_abi_records, omnipq_entry_point_signatures), not parsed from a header
RowPlanArg = _ext.struct("omnipq_row_plan")
PLAN_AWARE = _ext.PLAN_AWARE


# Measuring the SA stages INSIDE the replayed step.  A hipGraph replay cannot host timing events
# (torch refuses external events on ROCm), so the spans are made visible to a kernel trace instead: with SPAN_MARKERS set
# (bench.py --sa-markers; env OMNIPQ_SA_MARKERS=1) every "@sa" span -- ball query, fused forward, fused backward of each of the
# five stages, and the grouped weight-gradient launch: 16 per step -- starts and ends with a one-wave marker kernel
# (omnipq::sa_span_begin_kernel / _end_kernel) on the stream the span's kernels are launched on.  Captured with the step the
# markers are graph nodes in stream order, so in a `rocprofv3 --kernel-trace` of the replays the kernels of a span are exactly
# those between its two markers on the markers' queue (tools/sa_replay_timing.py -> profiles/r*_sa_stage_replay_timing.json,
# which bench.py reports as `roofline.replayed_step`).  Off in the product path and in every timed run.
SPAN_MARKERS = os.environ.get("OMNIPQ_SA_MARKERS") == "1"


class _tagged:
    """Label the timing-sink entries of everything launched inside (bench.py's per-stage accounting)."""

    def __init__(self, tag, stage=None):
        self.tag = tag
        self.stage = stage            # "@sa" spans: which stage (bench.py's per-stage split: sink names read "<call>@<stage>@sa")
        self.marked = False

    def __enter__(self):
        self.prev = _ext.timing_tag
        _ext.timing_tag = ("@" + self.stage + self.tag) if self.stage else self.tag
        if SPAN_MARKERS and self.tag == "@sa" and torch.cuda.is_available():
            self.marked = True
            _lib.omnipq_span_marker(0, _ext._stream())

    def __exit__(self, *exc):
        _ext.timing_tag = self.prev
        if self.marked:
            self.marked = False
            _lib.omnipq_span_marker(1, _ext._stream())


def _world():
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


_NBT = None        # None: bump BatchNorm step counters at once; list: collect them, one multi-tensor add at exit


def bump(nbt):
    """num_batches_tracked += 1 (state_dict parity with torch's BatchNorm), batched when a model asks for it."""
    if nbt is None:
        return
    if _NBT is None:
        nbt += 1
    else:
        _NBT.append(nbt)


class deferred_counters:
    """Within the block, the `num_batches_tracked` increments of every BatchNorm layer run by the hand-written
    kernels are collected and applied with ONE multi-tensor launch at exit (61 tiny launches per step otherwise)."""

    def __enter__(self):
        global _NBT
        self.outer = _NBT
        if _NBT is None:
            _NBT = []
        return self

    def __exit__(self, *exc):
        global _NBT
        if self.outer is None:
            pending, _NBT = _NBT, None
            if pending:
                torch._foreach_add_(pending, 1)
        return False


COLLECTIVES = 0                  # SyncBatchNorm statistics all-reduces issued so far by the hand-written kernels' host code
COLLECTIVES_LAST_STEP = 0        # ... during the last PQ_Transformer forward + backward (set by deferred_wgrads.__exit__)
_COLLECTIVES_MARK = 0
_FORCE_COLLECTIVES = False       # test hook: issue the SyncBatchNorm all-reduces even over a 1-rank group
IPC_STATS = None                 # an ipc_stats.IpcStats: the statistics exchange as peer-to-peer launches instead of RCCL (opt-in)


def _allreduce_(sums, world=None):
    """SyncBatchNorm's statistics exchange; `world` = the participant count the caller computed (1: this layer keeps
    per-rank statistics -- a plain BatchNorm under DDP)."""
    if world is None:
        world = _world()
    if world > 1 or (_FORCE_COLLECTIVES and dist.is_initialized()):
        global COLLECTIVES
        COLLECTIVES += 1
        if IPC_STATS is not None and sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous():
            IPC_STATS.allreduce_(sums)            # one launch, no RCCL (omni-pq_amd/ipc_stats.py; opt-in)
        else:
            dist.all_reduce(sums)
    return sums


class PairStats:
    """SyncBatchNorm statistics of the two stacks of a pair launch (rows_mlp._lockstep) in ONE buffer, exchanged by ONE
    all-reduce: the leading stack allocates [its rows | the partner's rows], the partner -- whose GEMM of the same kind goes
    out in the same grid -- takes the second half, and the leader, which resumes first, reduces both.  A partner that does not
    show up (different widths, a stack that ended) leaves the leader with a collective of its own."""
    active = None                  # the lockstep run in progress on this thread's stream, if any

    def __init__(self):
        self.slot = None

    class _Slot:
        __slots__ = ("buf", "rows", "joined", "reduced", "stash")

    def take(self, lead, rows, cols, device):
        """-> (f64 zeros [rows][cols], slot or None)"""
        if lead:
            s = self.slot = PairStats._Slot()
            s.buf, s.rows, s.joined, s.reduced, s.stash = zeros_f64(2 * rows, cols, device), rows, False, False, None
            return s.buf[:rows], s
        s = self.slot
        if s is not None and not s.joined and not s.reduced and tuple(s.buf.shape) == (2 * rows, cols):
            s.joined = True
            return s.buf[rows:], s
        return zeros_f64(rows, cols, device), None


def pair_sums(lead, rows, cols, device, world):
    """Statistics buffer of a BatchNorm layer; shared with the partner stack when a pair is running under a process group."""
    bus = PairStats.active
    if bus is None or not (world > 1 or _FORCE_COLLECTIVES):
        return zeros_f64(rows, cols, device), None
    return bus.take(lead, rows, cols, device)


def pair_allreduce(sums, slot, lead, world, before_partner=None):
    """`_allreduce_(sums)`, once for both stacks of a pair.  before_partner(partner's half) runs on the partner's LOCAL
    totals before they are replaced by the global ones (the BatchNorm backward takes its per-rank affine gradients from them)
    and its result is handed to the partner.  -> what before_partner returned for this stack, if it was run on its behalf."""
    if slot is None:
        _allreduce_(sums, world)
        return None
    if lead:
        if slot.joined:
            if before_partner is not None:
                slot.stash = before_partner(slot.buf[slot.rows:])
            _allreduce_(slot.buf, world)
            slot.reduced = True
        else:
            slot.reduced = True              # closes the slot: a late partner reduces on its own
            _allreduce_(sums, world)
        return None
    if slot.reduced and slot.joined:
        return slot.stash if before_partner is not None else None
    _allreduce_(sums, world)
    return None


def _round_up(x, q):
    return (x + q - 1) // q * q


def _gemm_nt(A, B, M, N, K):
    """bf16 C[M][N] = A[M][K] B[N][K]^T"""
    C = torch.empty((M, N), device=A.device, dtype=E16.dtype)
    _call(_lib.omnipq_gemm_nt_e16, A, M, N, K, _p(A), K, _p(B), K, _p(C), N)
    return C


def gemm_nt_into(A, B, C, M, N, K, bias=None):
    """C (bf16 [M][N], preallocated) = A[M][K] B[N][K]^T (+ bias); long contractions over few tiles get a
    split-K workspace."""
    n_ws = int(_lib.omnipq_gemm_nt_workspace_floats(M, N, K))
    ws = torch.empty((n_ws,), device=A.device, dtype=torch.float32) if n_ws else None
    _call(_lib.omnipq_gemm_nt_e16_ws, A, M, N, K, _p(A), K, _p(B), K, _p(C), N, _p(bias), _p(ws))


def _stats_workspace(M, N, device):
    """the partial-sum workspace of a statistics GEMM over M rows (omnipq_gemm_nt_stats_workspace_floats); None for the row
    counts whose statistics go straight to f64 atomics"""
    n_ws = int(_lib.omnipq_gemm_nt_stats_workspace_floats(M, N))
    return torch.empty((n_ws,), device=device, dtype=torch.float32) if n_ws else None


@functools.lru_cache(maxsize=None)
def _partial_sum_rows(P):
    """P rows take the statistics GEMMs' partial-sum path (the threshold is the library's: csrc/gemm_bf16.hip,
    kStatsDirectTiles); cached: the eager step asks once per row count, not once per stage"""
    return int(_lib.omnipq_gemm_nt_stats_workspace_floats(P, 8)) > 0


class Finalize(collections.namedtuple("Finalize", "sums count gamma beta eps momentum running_mean running_var conv_bias",
                                      defaults=(None,))):
    """What the launch that reads a training BatchNorm layer's constants first forms them from (`lay.fin`: the first consumer
    finalises and clears it).  conv_bias: what a preceding linear layer would add (only the running mean sees it)."""

    def tail(self):
        """the argument run every finalising entry point shares; its head is the call site's (include/omnipq_sa.h: the GEMM
        prologues and the pool-select launch take `sums, count`, omnipq_bn_finalize / _relu take `count, sums`)"""
        return _p(self.gamma), _p(self.beta), self.eps, self.momentum, _p(self.running_mean), _p(self.running_var)


class BallExtrema(collections.namedtuple("BallExtrema", "per ymax ymin amax amin")):
    """The extrema of every `per` consecutive rows (a ball, or a group of a planned stage's compact row space) that the last GEMM
    records per column (csrc/gemm_bf16.hip: PoolOut): values and the rows that attain them."""

    def args(self):
        return _p(self.ymax), _p(self.ymin), _p(self.amax), _p(self.amin)


def _gemm_nt_stats(A, B, M, N, K, sums, bias=None, pool=None):
    """bf16 C = A B^T and, in the same pass, sums (f64 [2][N], zero on entry) += column sum / sum of squares;
    pool (a BallExtrema): also the extrema of every ball."""
    C = torch.empty((M, N), device=A.device, dtype=E16.dtype)
    ws = _stats_workspace(M, N, A.device)
    if pool is not None:
        _call(_lib.omnipq_gemm_nt_e16_stats_pool, A, M, N, K, _p(A), K, _p(B), K, _p(C), N, _p(bias), _p(sums), _p(ws),
              pool.per, *pool.args())
        return C
    _call(_lib.omnipq_gemm_nt_e16_stats, A, M, N, K, _p(A), K, _p(B), K, _p(C), N, _p(bias), _p(sums), _p(ws))
    return C


# Conv+BN+ReLU stacks without stored activations: the consumer GEMMs rebuild X = relu(a y + b) from the layer's
# pre-BN output while staging their operand (csrc: AffineIn / AFFB).  AFFINE_OPERANDS = False restores the separate
# normalise+ReLU pass (kept for the parity tests).
AFFINE_OPERANDS = True


def affine_pays(P, N):
    """Rebuilding relu(bn(Y)) inside the consumer GEMMs costs VALU work per staged element, once per N-tile of the
    consumer; it saves the normalise+ReLU pass (a read and a write of the layer) and, with the finalize folded into
    the consumer's prologue, two launches per BatchNorm layer.  Measured on P x K rows (forward GEMM with the
    transform vs without | the pass it replaces): P = 1 M, K = 128, N = 128: +53 us | 106 us; N = 256: +46 | 106;
    P = 262 k, K = 256, N = 256: +18 | 40; N = 512: +34 | 40; P = 65 k, N = 512: +9 | 11; 4096 x 288 x 288: +2 | 6.
    So it pays everywhere on this model (with the scale / shift vectors in LDS; when they were fetched per K-step it
    lost on the wide layers).  AFFINE_OPERANDS = False restores the stored dataflow (parity tests)."""
    return AFFINE_OPERANDS


# inside deferred_wgrads the SA stages' weight gradients run as ONE grouped launch when the block ends (False: one
# GEMM + slab reduction per layer, as outside the block)
SA_WGRADS_GROUPED = True
POOL_EPILOGUE = True


# Row plan (csrc/common.h: RowPlan, include/omnipq_sa.h: omnipq_sa_ball_plan).  ball_query pads a ball that holds fewer than
# nsample points with copies of its first neighbour (ball_query_gpu.cu:36-45; pointnet2_utils.py:317-376 groups them like any
# other index), so the shared MLP of the reference runs on duplicate rows: on the benchmark's 40 000-point room scenes a ball
# of sa1 (radius 0.2, nsample 64) holds 27 real neighbours on average and a ball of sa2 (0.4, 32) seven (tools/ball_fill.py).
# A planned stage keeps, per ball, its first G * ceil(real neighbours / G) rows (G = PLAN_GROUP = 8: the finest unit the
# extrema epilogue of the GEMMs resolves), packs the balls' rows back to back (COMPACT row space) and runs every kernel on
# that: 48 % of sa1's rows and 31 % of sa2's on those scenes (54 % / 50 % with groups of 16).  The number of rows in use is
# data-dependent, so it lives in device memory and the launches keep the static grids of the full row count -- workgroups
# past it leave at once -- which keeps the step capturable into a hipGraph.  The dropped rows are accounted for exactly: they
# are copies of their ball's first row, so BatchNorm statistics weight that row by 1 + dropped copies, the max-pool is
# unchanged (a copy never beats the first row under the first-row tie rule), and in backward every copy contributes the
# constant term -a (m1 + yhat m2) of the BatchNorm backward once, i.e. (1 + copies) times on the first row; everything
# downstream (data gradients, weight gradients, BatchNorm-backward sums) is linear in those rows.  Results equal the full
# computation up to the order of the f32 sums (tests/test_gpu_fused_sa.py::test_row_plan_equals_the_full_stage).
# ROW_PLAN = False: every row is computed.
ROW_PLAN = True
PLAN_GROUP = 8                  # rows per group of a plan: 8 or 16
ONE_SIDED_EXTREMA = True        # planned stages with 8-row groups: record max OR min per column, by the sign of gamma
# (A BatchNorm weight of EXACTLY zero makes every row of a ball tie after BatchNorm + ReLU; the reference's max-pool then picks
# row 0, the extrema paths -- one- and two-sided -- the first row that attains the raw maximum.  The pooled VALUE is the same
# (relu(beta)), the gradient of that gamma differs by the choice of yhat; a weight does not sit at exactly 0.0 during training,
# and nothing else depends on the choice.  ADVICE r4.)
PLAN_MIN_ROWS = 1 << 17         # grouped rows from which a stage is planned (BASELINE configs[3], batch 4: sa2 has 2^17 --
                                # SA stages 2.65 -> 2.28 ms there; below that the statistics take the direct-atomics paths)
row_plan_uses = 0
KEEP_LAST_PLANS = False         # diagnostics (bench.py sets it): remember the latest plan of every stage size in row_plan_last
row_plan_last = {}              # P of the stage -> its latest _Plan, only while KEEP_LAST_PLANS (a kept plan pins its tensors --
                                # inside a captured step: blocks of the graph's memory pool -- for as long as it is the latest)


def row_plan_ok(training, S, P, L, needs_input_grad, pooled):
    """at least two 16-row blocks per ball, the partial-sum kernel paths (many rows), the dataflow without stored activations
    and with the ball extrema in the last GEMM (the kernels that know the plan), no gradient into the stage's coordinates (the
    centre-gradient kernel does not know it; feature gradients: the caller also asks for at most 8192 source points, the CSR
    builders that do)"""
    return ROW_PLAN and training and S in (32, 64, 128) and P >= PLAN_MIN_ROWS and P % 128 == 0 and L >= 2 and \
        AFFINE_OPERANDS and POOL_EPILOGUE and pooled and not needs_input_grad


class _Plan:
    __slots__ = ("goff", "rows_dev", "row_w", "scratch", "gs", "unit_src")


def plan_static_ok(S, P):
    """the part of row_plan_ok that depends on the stage's geometry only (what a plan made AHEAD of the stage can check)"""
    return ROW_PLAN and S in (32, 64, 128) and P >= PLAN_MIN_ROWS and P % 128 == 0


def plan_words(B, M, P):
    """int32 words of a plan's device state, each piece a multiple of 4 words: goff | rows_dev | unit_src | row_w"""
    r4 = lambda n: (n + 3) // 4 * 4
    return r4(B * M + 1), 4, r4(P // 8), r4(P // 4)


def make_row_plan(idx, P, into=None):
    """idx (B, M, S) int32 -> the stage's _Plan (three tiny launches).  into: a flat int32 tensor of sum(plan_words) words
    that receives the plan's state (a plan made ahead of its stage, in persistent memory: Pointnet2Backbone's sampling chain)"""
    B, M, S = idx.shape
    dev = idx.device
    plan = _Plan()
    plan.gs = PLAN_GROUP
    if into is None:
        plan.goff = torch.empty((B * M + 1,), device=dev, dtype=torch.int32)
        plan.rows_dev = torch.empty((1,), device=dev, dtype=torch.int32)
        plan.row_w = torch.empty((P,), device=dev, dtype=torch.uint8)
        plan.unit_src = torch.empty((P // 8,), device=dev, dtype=torch.int32)
    else:
        plan.goff, plan.rows_dev, plan.unit_src, plan.row_w = plan_views(into, B, M, P)
    plan.scratch = torch.empty((B * M,), device=dev, dtype=torch.int32)
    _call(_lib.omnipq_sa_ball_plan_src, idx, B * M, S, plan.gs, _p(idx), _p(plan.goff), _p(plan.rows_dev),
          _p(plan.row_w), _p(plan.unit_src), _p(plan.scratch))
    if KEEP_LAST_PLANS:
        row_plan_last[P] = plan
    return plan


def plan_views(flat, B, M, P):
    """the four tensors of a plan inside its flat int32 state (plan_words)"""
    w = plan_words(B, M, P)
    o1, o2, o3 = w[0], w[0] + w[1], w[0] + w[1] + w[2]
    return flat[:B * M + 1], flat[o1:o1 + 1], flat[o2:o2 + P // 8], flat[o3:o3 + w[3]].view(torch.uint8)[:P]


def build_csr_ahead(idx, N, plan, offsets, order):
    """The CSR of a stage's backward (omnipq_sa_build_csr) made ahead of the stage, in the row space of `plan` (None: every
    row), into given (B, N + 1) / (B, M * S) int32 tensors."""
    B, M, S = idx.shape
    scratch = torch.empty((B, N), device=idx.device, dtype=torch.int32)
    with _row_plan(plan, B * M * S):
        _call(_lib.omnipq_sa_build_csr, idx, B, N, M, S, _p(idx), _p(offsets), _p(order), _p(scratch))


def _csr_of(pre, idx, B, N, M, S, plan, anchor):
    """(offsets, order) of the stage's backward: `pre`, the chain_plan.Csr made ahead of the stage (run(group=)), if it was
    made in the row space this backward runs in -- the SAME plan state (its goff words and group size), or no plan on both
    sides (a flag alone let a CSR of another row space through when a switch changed between prefetch and
    forward) -- else built now (inside the caller's _row_plan block)."""
    space = None if plan is None else (plan.goff.data_ptr(), plan.gs)
    if pre is not None and pre.space == space and tuple(pre.offsets.shape) == (B, N + 1) and \
            tuple(pre.order.shape) == (B, M * S):
        return pre.offsets, pre.order
    dev = idx.device
    offsets = torch.empty((B, N + 1), device=dev, dtype=torch.int32)
    order = torch.empty((B, M * S), device=dev, dtype=torch.int32)
    scratch = torch.empty((B, N), device=dev, dtype=torch.int32)
    _call(_lib.omnipq_sa_build_csr, anchor, B, N, M, S, _p(idx), _p(offsets), _p(order), _p(scratch))
    return offsets, order


def plan_from_state(flat, B, M, P):
    """a _Plan over state some earlier launch wrote (a copy of what make_row_plan(into=) filled)"""
    plan = _Plan()
    plan.gs = PLAN_GROUP
    plan.goff, plan.rows_dev, plan.unit_src, plan.row_w = plan_views(flat, B, M, P)
    plan.scratch = None
    if KEEP_LAST_PLANS:
        row_plan_last[P] = plan
    return plan


class _PlanState(threading.local):       # per Python thread (forward thread / autograd thread): which plan _call passes
    arg = None                           # ctypes pointer to a RowPlanArg (which it keeps alive), or None


_plan_state = _PlanState()


class _row_plan:
    """The launches inside the block get `plan` (plan-aware entry points: as their `plan` argument, see _call).  pool_gamma:
    the plan also says that the ball extrema hold only the side this gamma's sign selects (omnipq_row_plan.pool_gamma) -- for
    the launches of THIS block: the struct is built on entry and not written afterwards."""

    def __init__(self, plan, rows, pool_gamma=None):
        self.plan, self.rows, self.pool_gamma = plan, rows, pool_gamma

    def __enter__(self):
        self.prev = _plan_state.arg
        plan = self.plan
        _plan_state.arg = None if plan is None else ctypes.pointer(RowPlanArg(
            _p(plan.rows_dev).value, _p(plan.row_w).value, _p(plan.goff).value, self.rows, plan.gs, _p(self.pool_gamma).value))

    def __exit__(self, *exc):
        _plan_state.arg = self.prev


def gemm_nt_affine(Y, below, Bw, M, N, K, sums=None, bias=None, out=None, pool=None, store=True):
    """bf16 C = relu(below.a * Y + below.b) Bw^T (+ bias); sums (f64 [2][N], zero on entry): also C's statistics.
    store=False (with pool, on a plan): C is not written -- statistics and ball extrema only; returns None."""
    C = (torch.empty((M, N), device=Y.device, dtype=E16.dtype) if out is None else out) if store else None
    ws = _stats_workspace(M, N, Y.device) if sums is not None else None
    fin = getattr(below, "fin", None)
    if fin is not None:
        # the layer below has not been finalised yet: this GEMM's prologue derives a / b from its totals (and stores
        # them, with mean / invstd and the running-statistics update) -- one launch less per BatchNorm layer
        below.fin = None
        head = (Y, M, N, K, _p(Y), K, _p(fin.sums), fin.count, *fin.tail(), _p(fin.conv_bias), _p(below.a), _p(below.b),
                _p(below.mean), _p(below.invstd), _p(Bw), K, _p(C), N, _p(bias), _p(sums), _p(ws))
        if pool is not None:
            _call(_lib.omnipq_gemm_nt_e16_bnaffine_pool, *head, pool.per, *pool.args())
        else:
            _call(_lib.omnipq_gemm_nt_e16_bnaffine, *head)
        return C
    if pool is not None:
        raise RuntimeError("gemm_nt_affine: ball extrema need the layer below to be finalised in the prologue")
    _call(_lib.omnipq_gemm_nt_e16_affine, Y, M, N, K, _p(Y), K, _p(below.a), _p(below.b), _p(Bw), K, _p(C), N,
          _p(bias), _p(sums), _p(ws))
    return C


# The first layer of a coordinates-only stage (sa1: conv 3 -> 128 over 1 M grouped positions) without its output: its
# consumers recompute y = W0 . x0 from the grouped coordinates (three FMAs per element), its BatchNorm statistics and its
# weight gradient follow from the moments of x0 (csrc/xyz_layer.hip, gemm_bf16.hip: XyzGen).  Per step on sa1 this removes
# one write and four reads of Y1, the write and read of dz1, of dY1, and two GEMM launches: 2.4 GB of 7.8 GB.
# XYZGEN = False restores the stored first layer (tests compare the two).
XYZGEN = True
xyzgen_uses = 0            # forwards that took the path (tests check that it is the one that ran)


def xyzgen_ok(P, L, c0, needs_input_grad):
    """first layer generated from coordinates: training, no features, at least three layers (the second is not the pooled
    one), the row counts of the kernels' partial-sum path, no gradient into the coordinates"""
    return XYZGEN and L >= 3 and _partial_sum_rows(P) and c0 <= 256 and c0 % 8 == 0 and not needs_input_grad


# The first layer of a stage WITH features on the SOURCE points (round 5; include/omnipq_sa.h: omnipq_sa_l1_rows).  The first
# conv is linear in the grouped row [features(idx) | xrel], so it commutes with the grouping: Z = features W_f^T once per
# source point -- a point is read by 4 (vote aggregation) to 16 (sa2) balls, so the contraction runs over 4 .. 16 times fewer
# rows -- then y = Z[idx] + W_x . xrel per grouped row (gather + 3 FMAs + the statistics, one streaming launch).  The grouped
# input rows X0 (sa2: 151 MB, written once and read twice per step) never exist; in backward the rows of dY1 are summed per
# point first (the CSR scatter, now over C1 channels instead of cin + 3), and the weight gradient and the feature gradient
# are contractions over the points.  Same values up to the order of the f32 sums (one e16 rounding of y, as before).
# HOIST_L1 = False restores the grouped first layer (tests compare the two).
HOIST_L1 = True
hoist_uses = 0


def hoist_ok(training, features, cin, cin_raw, L, c1, xgen):
    return HOIST_L1 and training and features is not None and not xgen and cin == cin_raw and cin % 32 == 0 and cin > 0 and \
        L >= 2 and AFFINE_OPERANDS and c1 % 32 == 0 and 32 <= c1 <= 640


# The LAST layer of a planned stage, backward without its output gradient (round 6; csrc/sa_last_bwd.hip):
# dY3 = a hit - w (alpha + beta Y3) with Y3 = X2 W3^T substituted, so that dX2 and dW3 are contractions of X2 (rebuilt from Y2
# as everywhere), the one-hot pool gradient `hit` (generated inside the two GEMMs from one word per ball and column) and
# C2-sized matrices.  Neither dY3 nor Y3 exists: the forward's last GEMM stores statistics and ball extrema only.
# LAST_NO_DY = False restores the stored Y3 / dY3 (tests/test_gpu_last_no_dy.py and tests/test_gpu_fused_sa.py compare the two).
LAST_NO_DY = True
LAST_NO_DY_MAX_C3 = 256         # ... for last layers up to this width: sa1 (128 -> 256) gains ~20 us per step, sa2 (256 -> 512: 12 + 16
                                # K-steps in the data-gradient GEMM, six 128 x 128 tiles per slab in the weight gradient) LOSES
                                # 30-90 us (per-stage split of the bench line: sa2 0.69 -> 0.78 ms with it); 1 << 30 = every planned stage
LAST_X2 = True                  # ... and its weight gradient contracts X2 as the data-gradient launch left it (no affine per fragment)
last_no_dy_uses = 0


def last_no_dy_ok(plan, L, P, c2, c3, S, below_keeps_y_only):
    """a plan with its unit map, the layer below consumed as (Y, a, b), whole 128-column tiles on both sides, and more
    row tiles than the statistics take straight to f64 atomics (P rows on the partial-sum path, as omnipq_gemm_nt_e16_dz_bnbwd
    and the no-store omnipq_gemm_nt_e16_bnaffine_pool require)"""
    return LAST_NO_DY and c3 <= LAST_NO_DY_MAX_C3 and plan is not None and getattr(plan, "unit_src", None) is not None and L >= 2 and \
        _partial_sum_rows(P) and below_keeps_y_only and c2 % 128 == 0 and c3 % 128 == 0 and c2 + 32 <= 1024 and S >= 8 and \
        (S & (S - 1)) == 0 and AFFINE_OPERANDS and POOL_EPILOGUE


# The INFERENCE stage in one launch (csrc/sa_infer.hip, include/omnipq_sa.h: omnipq_sa_infer).  In eval mode
# BatchNorm is the affine a = gamma / sqrt(running_var + eps), b = beta - running_mean a, known before the launch, so no
# grid-wide statistics sit between a layer's GEMM and its consumer: a tile of balls goes from point indices to pooled features
# inside one workgroup -- gather, up to three conv + folded BatchNorm + ReLU layers and the max-pool -- and nothing of shape
# [P][.] is written.  Taken when nothing can ask for a backward: eval mode, run() called under torch.no_grad().
# EVAL_CHAIN = False restores the stored dataflow (gather, one GEMM + normalise/ReLU pass per layer, pool).
EVAL_CHAIN = True
eval_chain_uses = 0
_InferLayer = _ext.sa_infer_layer_struct()


@functools.lru_cache(maxsize=None)
def _infer_lds_bytes(S, kpad, widths):
    return int(_lib.omnipq_sa_infer_lds_bytes(S, kpad, len(widths), (ctypes.c_int * len(widths))(*widths)))


def eval_chain_ok(S, kpad, widths):
    """the shapes omnipq_sa_infer takes (nsample 16 / 32 / 64 / 128, one to three layers of 32 k <= 640 channels, kpad % 32 == 0
    and an LDS footprint the CU has): asked of the library, which refuses exactly the others"""
    return _infer_lds_bytes(int(S), int(kpad), tuple(int(w) for w in widths)) > 0


def last_wgrad_dz(Y2, below, hot, plan, S, C3, C2, P, alpha, beta, Wp, out=None):
    """dW3 (f32 [C3][C2]) of a stage's last layer from the layer below's pre-BN output (below is None: from X2 = relu(bn(.))
    itself, as the data-gradient launch left it) and the pool's one-hot gradient (omnipq_gemm_tn_dz +
    omnipq_sa_last_wgrad_combine); inside the caller's _row_plan block."""
    dev = Y2.device
    ws = torch.empty((int(_lib.omnipq_gemm_tn_dz_workspace_floats(C3, C2, P)),), device=dev, dtype=torch.float32)
    slabs, cs_off = ctypes.c_int(0), ctypes.c_longlong(0)
    _call(_lib.omnipq_gemm_tn_dz, Y2, C3, C2, P, _p(Y2), Y2.stride(0), _p(below.a if below is not None else None),
          _p(below.b if below is not None else None), _p(hot), _p(plan.unit_src), S, _p(ws), ctypes.byref(slabs),
          ctypes.byref(cs_off))
    if out is None:
        out = torch.empty((C3, C2), device=dev, dtype=torch.float32)
    _call(_lib.omnipq_sa_last_wgrad_combine, Y2, C3, C2, _p(ws), ctypes.c_void_p(ws.data_ptr() + 4 * cs_off.value),
          slabs.value, C3 + C2, _p(alpha), _p(beta), _p(Wp), Wp.stride(0), _p(out), C2, 0)
    return out


def gemm_nt_f32(A, B, M, N, K, lda, ldb):
    """f32 C[M][N] = A[M][K] B[N][K]^T (16-bit operands, whole contraction per tile)"""
    C = torch.empty((M, N), device=A.device, dtype=torch.float32)
    _call(_lib.omnipq_gemm_nt_e16_f32, A, M, N, K, _p(A), lda, _p(B), ldb, _p(C), N)
    return C


def gemm_nt_xyz(X0c, below, Bw, M, N, K, sums):
    """bf16 C = relu(bn(X0c W0^T)) Bw^T + its statistics: `below` is the never-materialised first layer (Wp, fin)."""
    C = torch.empty((M, N), device=X0c.device, dtype=E16.dtype)
    ws = _stats_workspace(M, N, X0c.device)
    below.fin, fin = None, below.fin                 # the first consumer finalises
    _call(_lib.omnipq_gemm_nt_e16_xyz_bnaffine, X0c, M, N, K, _p(X0c), X0c.shape[1], _p(below.Wp), below.Wp.shape[1],
          _p(fin.sums), fin.count, *fin.tail(), _p(below.a), _p(below.b), _p(below.mean), _p(below.invstd), _p(Bw), K, _p(C), N,
          _p(sums), _p(ws))
    return C


def _gemm_nt_bnbwd(dY, Wt, M, N, K, below, sums):
    """dX = dY Wt^T (bf16 [M][N]) and, in the same pass, the BatchNorm-backward sums of the layer `below`
    (its pre-BN output Y and constants a, b, mean, invstd) into sums (f64 [>=2][N], zero on entry)."""
    C = torch.empty((M, N), device=dY.device, dtype=E16.dtype)
    ws = _stats_workspace(M, N, dY.device)
    _call(_lib.omnipq_gemm_nt_e16_bnbwd, dY, M, N, K, _p(dY), K, _p(Wt), K, _p(C), N, _p(below.Y), _p(below.a),
          _p(below.b), _p(below.mean), _p(below.invstd), _p(sums), _p(ws))
    return C


def _gemm_tn(A, B, M, N, P, colsum=None, below=None):
    """f32 C[M][N] = A[P][M]^T B[P][N]; colsum (f32 [M], zero on entry): also += column sums of A;
    below: B is that layer's pre-BN output and stands for relu(below.a * B + below.b)"""
    C = torch.empty((M, N), device=A.device, dtype=torch.float32)
    ws = torch.empty((int(_lib.omnipq_gemm_tn_workspace_floats(M, N, P)),), device=A.device, dtype=torch.float32)
    if below is not None:
        _call(_lib.omnipq_gemm_tn_e16_affine, A, M, N, P, _p(A), M, _p(B), N, _p(below.a), _p(below.b), _p(C), _p(ws),
              _p(colsum))
    elif colsum is None:
        _call(_lib.omnipq_gemm_tn_e16, A, M, N, P, _p(A), M, _p(B), N, _p(C), _p(ws))
    else:
        _call(_lib.omnipq_gemm_tn_e16_colsum, A, M, N, P, _p(A), M, _p(B), N, _p(C), _p(ws), _p(colsum))
    return C


_TnProblem = _ext.struct("omnipq_tn_problem")


def empty_f32(shape, device):
    """the deferred weight gradients' memory that nothing clears (tests poison it)"""
    return torch.empty(shape, device=device, dtype=torch.float32)


def _plan_buffer(b, dev):
    """a wgrads.Buffer in device memory: in its parameter's shape and on its device, scratch flat"""
    shape, device = ((b.numel,), dev) if b.param is None else (b.param.shape, b.param.device)
    if b.kind == "empty":
        return empty_f32(shape, device)
    if b.kind == "pooled":
        return zeros_f32(b.numel, device).view(shape)
    return torch.zeros(shape, device=device, dtype=torch.float32)


class deferred_wgrads:
    """`with deferred_wgrads(): loss.backward()` -- inside the block the rows engine does not launch the weight
    (and bias) gradient of a linear layer whose weight is a Parameter (a row range of one, or a cat_params of
    several) when its turn comes in backward: it records the operands, returns no gradient to autograd, and at
    exit ALL recorded gradients are computed by one grouped launch (csrc/gemm_tn_bf16.hip) and stored /
    accumulated into `.grad` exactly as AccumulateGrad would have done.  Nothing reads a weight gradient before
    the optimizer, so the result is the same; what changes is ~350 launches of 5-25 us becoming a handful.
    Tensor hooks on those parameters do not fire (DistributedDataParallel relies on them: do not combine the
    two)."""
    active = None

    def __init__(self, on_early_flush=None):
        """on_early_flush(dfr): called on the side stream right after an early flush (`flush_on`) has launched -- the
        gradients collected up to that point are final; data_parallel.GradientBuckets starts their all-reduce there."""
        self.on_early_flush = on_early_flush

    def __enter__(self):
        if deferred_wgrads.active is not None:
            raise RuntimeError("deferred_wgrads blocks do not nest")
        self.items = []             # wgrads.Item: the per-point layers
        self.sa_items = []          # wgrads.Item: the SA stages' layers, a grouped launch of their own (see add_sa)
        self.ln_items = []          # (partials [blocks][2C], blocks, C, gamma, beta): LayerNorm parameter gradients
        self.dz_items = []          # (arguments of last_wgrad_dz, weight target, stage label): last layers without dY (LAST_NO_DY)
        self.producers = set()      # streams other than the flushing one on which collected operands were produced
        self._inflight = []         # what early flushes have launched on: alive until the block ends
        self._assign = []           # (parameter, f32 gradient) computed so far: `.grad` is touched when the block ends
        self._side_streams = []     # the streams early flushes ran on
        deferred_wgrads.active = self
        return self

    def _note_producer(self, t):
        """Operands are recorded on whatever stream their backward node runs on (the decoder's key sides have their own,
        models/decoder_rows.py: precompute_key_sides); a flush waits for those streams as well."""
        if t.is_cuda:
            self.producers.add(torch.cuda.current_stream(t.device))

    def add_layernorm(self, part, blocks, C, gamma, beta):
        """dgamma | dbeta of one LayerNorm as per-workgroup partial sums (omnipq_add_dropout_layernorm_bwd_partials)."""
        self._note_producer(part)
        self.ln_items.append((part, blocks, C, gamma, beta))

    def add(self, dY, X, M, N, P, wt, crop, bt, below=None):
        """below: X is that layer's pre-BN output and stands for relu(below.a * X + below.b)"""
        wgrads._refuse_ddp(wt)
        self._note_producer(dY)
        self.items.append(wgrads.Item(dY, X, M, N, P, wt, crop, bt, None if below is None else (below.a, below.b)))

    def add_sa(self, dY, X, M, N, P, wt, crop, below=None, blk=None):
        """A layer of a fused SA stage (up to a million positions): collected apart from the per-point layers and run
        as ONE grouped launch for all stages when the block ends.  One by one these GEMMs are split into ~512
        workgroups each -- two per CU, the launch's tail and its slab reduction paid 14 times per step; together
        they fill the chip with ~4000 workgroups cut for balance.  blk: the stage's row plan (_Plan), or None."""
        wgrads._refuse_ddp(wt)
        self._note_producer(dY)
        self.sa_items.append(wgrads.Item(dY, X, M, N, P, wt, crop, None, None if below is None else (below.a, below.b), blk))

    def add_dz(self, args, wt, stage):
        """The last layer of a planned SA stage (LAST_NO_DY): its weight gradient is launched with the other SA stages' when
        the block ends (last_wgrad_dz: its own launch, the operands are generated)."""
        wgrads._refuse_ddp(wt)
        self._note_producer(args[0])
        self.dz_items.append((args, wt, stage))

    def __exit__(self, et, ev, tb):
        deferred_wgrads.active = None
        global COLLECTIVES_LAST_STEP, _COLLECTIVES_MARK
        COLLECTIVES_LAST_STEP, _COLLECTIVES_MARK = COLLECTIVES - _COLLECTIVES_MARK, COLLECTIVES
        if et is None:
            self._wait_producers(None)
            self.flush()
        # early flushes run on side streams: join them on BOTH paths (after an exception their launches must not
        # outlive the operands this block releases below)
        for st in self._side_streams:
            torch.cuda.current_stream(st.device).wait_stream(st)
        if et is None:
            for param, g in self._assign:          # .grad is complete after the block
                self._accumulate(param, g)
        self.items = None
        self.sa_items = None
        self.dz_items = None
        self.ln_items = None
        self._inflight = None
        self._assign = None
        self._side_streams = None
        return False

    def _wait_producers(self, stream):
        """`stream` (None: the current one) waits for every stream operands were recorded on."""
        for ps in self.producers:
            st = stream if stream is not None else torch.cuda.current_stream(ps.device)
            if ps != st:
                st.wait_stream(ps)

    def flush_on(self, stream):
        """Compute what has been collected so far on `stream` (ordered after the current stream), e.g. the decoder's
        and heads' gradients underneath the backbone's backward pass.  Operands stay referenced until the block
        ends (they were allocated on the current stream's pool)."""
        if not self.items and not self.ln_items:
            return
        cur = torch.cuda.current_stream(stream.device)
        stream.wait_stream(cur)
        self._wait_producers(stream)
        self._inflight.extend(self.items)
        self._inflight.extend(self.ln_items)
        if stream not in self._side_streams:
            self._side_streams.append(stream)
        with torch.cuda.stream(stream):
            self.flush()
            self.items = []
            self.ln_items = []
            if self.on_early_flush is not None:
                self.on_early_flush(self)

    def _flush_layernorms(self):
        """All LayerNorm parameter gradients collected so far: ONE reduction launch per 32 of them into one flat
        zero-initialised buffer; the parameters get views of it when the block ends."""
        todo, self.ln_items = self.ln_items, []
        for i0 in range(0, len(todo), 32):
            chunk = todo[i0:i0 + 32]
            n = len(chunk)
            dev = chunk[0][0].device
            flat = zeros_f32(sum(2 * it[2] for it in chunk), dev)
            parts = (ctypes.c_void_p * n)(*[it[0].data_ptr() for it in chunk])
            blocks = (ctypes.c_int * n)(*[it[1] for it in chunk])
            chans = (ctypes.c_int * n)(*[it[2] for it in chunk])
            outs, off = (ctypes.c_void_p * n)(), 0
            for i, (_, _, C, gamma, beta) in enumerate(chunk):
                outs[i] = flat.data_ptr() + 4 * off
                self._assign.append((gamma, flat[off:off + C].view(gamma.shape)))
                self._assign.append((beta, flat[off + C:off + 2 * C].view(beta.shape)))
                off += 2 * C
            _call(_lib.omnipq_layernorm_param_reduce, flat, n, parts, blocks, chans, outs)
            self._inflight.extend(chunk)      # the partials stay alive until the block ends

    def flush(self):
        if self.ln_items:
            self._flush_layernorms()
        if self.items:
            self._flush_items(self.items)
        if deferred_wgrads.active is None:       # only when the block ends: every stage is in
            self._flush_sa()

    def _flush_sa(self):
        """The SA stages' layers collected so far: one grouped launch + one launch per last layer without dY."""
        if self.sa_items:
            items, self.sa_items = self.sa_items, []
            with _tagged("@sa"):
                self._flush_items(items)
            self._inflight.extend(items)
        if self.dz_items:
            todo, self.dz_items = self.dz_items, []
            for args, wt, stage in todo:
                Y2, below, hot, plan, S, C3, C2, P, alpha, beta, Wp = args
                with _tagged("@sa", stage), _row_plan(plan, P):
                    buf = last_wgrad_dz(Y2, below, hot, plan, S, C3, C2, P, alpha, beta, Wp)
                self._assign.append((wt.param, buf.view(wt.param.shape)))
            self._inflight.extend(todo)

    def _flush_items(self, items):
        """One grouped launch: wgrads.place() says where every gradient lands; allocate that, launch, add, note for .grad."""
        dev = items[0].dY.device
        plan = wgrads.place(items)
        bufs = [_plan_buffer(b, dev) for b in plan.buffers]

        def span(s):
            return bufs[s.buf].view(-1)[s.off:s.off + s.n]

        probs = (_TnProblem * len(items))()
        for q, it, pr in zip(probs, items, plan.problems):
            q.rows_dev = 0 if it.blk is None else it.blk.rows_dev.data_ptr()
            q.rot = pr.rot
            q.A, q.B = it.dY.data_ptr(), it.X.data_ptr()
            q.ba, q.bb = (0, 0) if it.aff is None else (it.aff[0].data_ptr(), it.aff[1].data_ptr())
            q.M, q.N, q.P, q.lda, q.ldb = it.M, it.N, it.P, it.dY.stride(0), it.X.stride(0)
            q.out_rows, q.out_cols, q.out_ld, q.flags = pr.out_rows, pr.out_cols, pr.out_ld, 0
            q.out = bufs[pr.out.buf].data_ptr() + 4 * pr.out.off
            q.colsum = 0 if pr.colsum is None else bufs[pr.colsum.buf].data_ptr() + 4 * pr.colsum.off
        ws = empty_f32((int(_lib.omnipq_gemm_tn_grouped_workspace_floats(len(items), ctypes.byref(probs))),), dev)
        _call(_lib.omnipq_gemm_tn_grouped, ws, len(items), ctypes.byref(probs), _p(ws))
        for dst, src in plan.adds:
            span(dst).add_(span(src))
        # `.grad` is touched only when the block ends (after the side streams have been joined): autograd may still
        # accumulate into the same parameter later in this backward pass, on the caller's stream
        for param, s in plan.assigns:
            whole = plan.buffers[s.buf].param is param
            self._assign.append((param, bufs[s.buf] if whole else span(s).view(param.shape)))

    @staticmethod
    def _accumulate(param, g):
        g = g if param.dtype == torch.float32 else g.to(param.dtype)
        if param.grad is None:
            param.grad = g
        else:
            param.grad.add_(g)


class WgradFlushPoint(torch.autograd.Function):
    """Identity in forward; when the gradient comes back through it inside a `deferred_wgrads` block, everything
    collected so far is launched on the side stream `stream_of()` returns (None: nothing happens)."""

    @staticmethod
    def forward(ctx, x, stream_of):
        ctx.e16 = E16.dtype
        ctx.stream_of = stream_of
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        E16.select(ctx.e16)
        dfr = deferred_wgrads.active
        if dfr is not None and g.is_cuda:
            st = ctx.stream_of()
            if st is not None:
                dfr.flush_on(st)
        return g, None


class _ZeroPool:
    """Zero-initialised scratch handed out in slices that are used once and never recycled: a chunk is
    cleared by ONE memset when it is allocated, instead of one memset per statistics buffer (a training
    step asks for ~200 of them).  A slice keeps its chunk alive; chunks are a few hundred KB.  One open chunk
    per (device, stream): its memset is ordered on that stream.  Chunks opened inside a graph capture are
    dropped when the capture state changes -- their memset node belongs to that graph only."""

    def __init__(self, dtype, chunk):
        self.dtype, self.chunk = dtype, chunk
        self.open = {}            # (device, stream) -> [buffer, used]
        self.capturing = False

    def reset(self):
        self.open.clear()

    def take(self, n, device):
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing != self.capturing:
            self.open.clear()
            self.capturing = capturing
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        n8 = _round_up(n, 16)
        slot = self.open.get(key)
        if slot is None or slot[1] + n8 > slot[0].numel():
            slot = [torch.zeros(max(self.chunk, n8), device=device, dtype=self.dtype), 0]
            self.open[key] = slot
        out = slot[0][slot[1]:slot[1] + n]
        slot[1] += n8
        return out


_ZEROS_F64 = _ZeroPool(torch.float64, 1 << 16)
_ZEROS_F32 = _ZeroPool(torch.float32, 1 << 15)


def reset_pools():
    """Forget the open chunks (call right before starting a graph capture)."""
    _ZEROS_F64.reset()
    _ZEROS_F32.reset()


def zeros_f64(rows, cols, device):
    return _ZEROS_F64.take(rows * cols, device).view(rows, cols)


def zeros_f32(n, device):
    return _ZEROS_F32.take(n, device)


class WeightArena:
    """Every weight matrix the hand-written GEMMs of a model use, prepared (padded / rotated bf16 copy and its
    transpose) by ONE launch per step instead of one per layer.

    The first forward inside `with arena.step(device):` records which matrices are asked for (`prep_weight`
    still prepares them one by one); from then on `step()` runs `omnipq_prep_weights_all` over the recorded
    table and `prep_weight` hands out views of the arenas.  Parameters are referenced, not copied: in-place
    optimizer updates are picked up by the next step's launch.  A matrix that was not recorded falls back to
    its own launch and is added for the following step."""

    def __init__(self):
        self.keys = {}            # key -> index
        self.entries = []         # (W2 view, cout, cin, ldw, cp, k, rot)
        self.views = []           # (Wp, Wt) per entry, valid while `active`
        self.built = 0            # number of entries the device table covers
        self.table = self.tiles = self.wp = self.wt = None
        self.total = 0
        self.active = False

    @staticmethod
    def _key(W2, cp, k, rot):
        return (W2.data_ptr(), tuple(W2.shape), W2.stride(0), cp, k, rot)

    def _build(self, device):
        import numpy as np
        rec = np.dtype([("W", "<u8"), ("wp", "<i8"), ("wt", "<i8"), ("first", "<i8"), ("cout", "<i4"), ("cin", "<i4"),
                        ("ldw", "<i4"), ("cp", "<i4"), ("k", "<i4"), ("rot", "<i4")])
        tab = np.zeros(len(self.entries), dtype=rec)
        off = 0
        for i, (W2, cout, cin, ldw, cp, k, rot) in enumerate(self.entries):
            tab[i] = (W2.data_ptr(), off, off, off, cout, cin, ldw, cp, k, rot)
            off += cp * k
        self.total = off
        tiles = [(i, r0, c0, 0) for i, (_, _, _, _, cp, k, _) in enumerate(self.entries)
                 for r0 in range(0, cp, 64) for c0 in range(0, k, 64)]
        self.tiles = torch.tensor(tiles, dtype=torch.int32).reshape(-1, 4).to(device)
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(device)
        self.wp = torch.empty(off, device=device, dtype=E16.dtype)
        self.wt = torch.empty(off, device=device, dtype=E16.dtype)
        self.views = []
        off = 0
        for (_, _, _, _, cp, k, _) in self.entries:
            self.views.append((self.wp[off:off + cp * k].view(cp, k), self.wt[off:off + cp * k].view(k, cp)))
            off += cp * k
        self.built = len(self.entries)

    def step(self, device):
        return _ArenaStep(self, device)

    def lookup(self, W2, cp, k, rot):
        i = self.keys.get(self._key(W2, cp, k, rot))
        if i is None or i >= self.built:
            return None
        return self.views[i]

    def record(self, W2, cp, k, rot):
        key = self._key(W2, cp, k, rot)
        if key not in self.keys:
            self.keys[key] = len(self.entries)
            self.entries.append((W2, W2.shape[0], W2.shape[1], W2.stride(0), cp, k, rot))


class _ArenaStep:
    def __init__(self, arena, device):
        self.arena, self.device = arena, device

    def __enter__(self):
        global _ARENA
        a = self.arena
        self.outer = _ARENA
        if torch.device(self.device).type != "cuda":
            return self
        if a.built and a.wp.dtype != E16.dtype:
            a.built = 0                        # the element type changed since the arenas were laid out
        if len(a.entries) != a.built and not torch.cuda.is_current_stream_capturing():
            a._build(self.device)              # table upload: never inside a capture
        if a.built:
            _call(_lib.omnipq_prep_weights_all, a.wp, a.built, int(a.tiles.shape[0]), _p(a.table), _p(a.tiles),
                  _p(a.wp), _p(a.wt))
        a.active = True
        _ARENA = a
        return self

    def __exit__(self, *exc):
        global _ARENA
        self.arena.active = False
        _ARENA = self.outer
        return False


_ARENA = None
_ARENAS = weakref.WeakKeyDictionary()      # model -> its WeightArena (kept out of the module: copies start afresh)


def arena_of(model):
    arena = _ARENAS.get(model)
    if arena is None:
        arena = _ARENAS[model] = WeightArena()
    return arena


def is_persistent(W):
    """A Parameter, a view of one, or a joint_params buffer: its storage (hence its address) outlives the step."""
    if getattr(W, "omnipq_persistent", False):
        return True
    root = W._base if W._base is not None else W
    return isinstance(root, torch.nn.Parameter)


def prep_weight(W2, cp, k, rot=0, transpose=True, persistent=False):
    """f32 (cout, cin) parameter -> bf16 [cp][k] (zero-padded, columns rotated left by rot) and its
    transpose [k][cp], in one launch -- or, inside a model's `WeightArena.step()`, views of the arenas that the
    step's single launch filled."""
    W2 = W2.detach()
    if W2.dtype != torch.float32 or W2.stride(1) != 1:
        W2 = W2.float().contiguous()
    elif persistent and _ARENA is not None and _ARENA.active:
        got = _ARENA.lookup(W2, cp, k, rot)
        if got is not None:
            return got
        _ARENA.record(W2, cp, k, rot)
    cout, cin = W2.shape
    Wp = torch.empty((cp, k), device=W2.device, dtype=E16.dtype)
    Wt = torch.empty((k, cp), device=W2.device, dtype=E16.dtype) if transpose else None
    _call(_lib.omnipq_prep_weight, W2, cout, cin, W2.stride(0), cp, k, rot, _p(W2), _p(Wp), _p(Wt))
    return Wp, Wt


def unprep_wgrad(dWp, cout, cin, rot, shape):
    """f32 [cp][k] gradient of the prepared weight -> gradient in the parameter's own shape."""
    cp, k = dWp.shape
    if cp == cout and k == cin and rot == 0:
        return dWp.view(shape)
    dW = torch.empty(shape, device=dWp.device, dtype=torch.float32)
    _call(_lib.omnipq_unprep_wgrad, dWp, cout, cin, k, rot, _p(dWp), _p(dW))
    return dW


def bn_backward_apply(d, lay, P, C, total, sums, world, out=None, pair=None):
    """d (gradient w.r.t. the ReLU output, bf16 [P][C]) -> gradient w.r.t. the layer's pre-BN output, written to
    `out` (default: in place), given the BatchNorm-backward totals `sums` of THIS rank.  Returns (dgamma, dbeta),
    this rank's share.
    Single process: one launch does the means, the f32 copies of the totals and the apply; under a process
    group the totals are all-reduced in between (SyncBatchNorm), so the local gradients are taken first."""
    if world > 1 or _FORCE_COLLECTIVES:
        slot, lead = pair if pair is not None else (None, False)
        if slot is not None and not lead and slot.joined and slot.reduced:
            dgamma, dbeta = slot.stash           # taken by the leader before its all-reduce covered both halves
        else:
            dgamma, dbeta = affine_grads(sums, C)
            if slot is None:
                _allreduce_(sums[:2], world)
            else:
                pair_allreduce(sums[:2], slot, lead, world, before_partner=lambda half: affine_grads(half, C))
        gb = None
    else:
        gb = torch.empty((2, C), device=d.device, dtype=torch.float32)
        dgamma, dbeta = gb[1], gb[0]
    _call(_lib.omnipq_bn_bwd_apply_fused, d, P, C, total, _p(d), _p(lay.Y), _p(lay.a), _p(lay.b),
          _p(lay.mean), _p(lay.invstd), _p(sums), _p(d if out is None else out), _p(gb))
    return dgamma, dbeta


def affine_grads(sums, C):
    """(dgamma, dbeta) f32 from the local f64 totals [sum dz | sum dz*yhat]."""
    both = torch.empty((2, C), device=sums.device, dtype=torch.float32)
    _call(_lib.omnipq_sums_to_f32, sums, C, _p(sums), _p(both[0]), _p(both[1]))
    return both[1], both[0]


def rows16_of(t, shape):
    """The position-major bf16 twin a producer attached to `t` (attribute `omnipq_rows16`: the same values as
    (B, n, C) bf16 data), if it is there and matches."""
    twin = getattr(t, "omnipq_rows16", None) if t is not None else None
    if twin is None or tuple(twin.shape) != tuple(shape) or twin.dtype != E16.dtype or not twin.is_contiguous():
        return None
    return twin


class _Layer:
    """Per-layer constants and saved tensors of one conv+BN+ReLU."""
    __slots__ = ("K", "C", "Wp", "Wt", "a", "b", "mean", "invstd", "Y", "X", "fin", "mom")


# Sizes of one stage pass.  P = B * M * S grouped rows; cin = cin_raw rounded up to 8 (feature rows are moved in 16-byte pieces:
# 6 extra input channels -- rgb + normals, BASELINE configs[3] -- travel as 8, the two extra columns and weight columns zero);
# kpad: the first layer's contraction length; world: the ranks its BatchNorm statistics are summed over
_Geom = collections.namedtuple("_Geom", "B N M S P cin cin_raw kpad inv_r world")


class StageRoute(typing.NamedTuple):
    """Every decision of one stage pass, made by stage_route() before anything is launched.  FusedSAStage._forward stores it
    on ctx; forward and backward dispatch on it and decide nothing themselves.  A new route is a new value of a field here, its
    condition in stage_route(), and a step function for the dispatchers (_forward_layers, FusedSAStage._backward) to call."""
    training: bool
    first: str        # layer 0: "grouped" (on the gathered rows [features | xyz]) | "xyz" (generated from the grouped coordinates,
                      # never stored: XYZGEN) | "source" (on the source points, gathered afterwards: HOIST_L1) | "chain" (the
                      # whole stage, gather to pool, is ONE forward-only launch: EVAL_CHAIN)
    plan_gs: int      # rows per group of the stage's row plan (ROW_PLAN); 0: every row is computed
    plan_arrives: bool    # the plan that came with idx is the stage's (else forward makes one)
    feed: tuple       # per layer below the last, what its consumers read: "stored" relu(bn(Y)) | "yab" (Y, a, b) (AFFINE_OPERANDS)
                      # | "lds" (the activation never leaves the workgroup: "chain")
    finalize: tuple   # per layer, where its BatchNorm is finalised: "launch" (its own) | "relu" (with the ReLU pass) | "consumer"
                      # (the prologue of the GEMM it feeds) | "pool" (the pool-select launch) | "running" (eval: nothing to do)
                      # | "folded" (eval, "chain": the kernel forms a / b from the running estimates itself)
    extrema: str      # ball extrema recorded by the last GEMM (POOL_EPILOGUE): "" (the pool scans Y) | "both" | "one" (the side
                      # gamma's sign selects: ONE_SIDED_EXTREMA)
    last: str         # the last layer's backward: "y" (statistics from the stored Y) | "ysel" (from the pooled rows' values) |
                      # "no_dy" (neither Y3 nor dY3 exists: LAST_NO_DY)
    keep_x2: bool     # "no_dy": the data-gradient launch leaves X2 for the weight gradient (LAST_X2)


def stage_route(training, B, N, M, S, cin_raw, widths, has_features, xyz_grad, feat_grad, plan_gs=None, plan_unit_map=False,
                no_grad=False):
    """The route of a stage from shapes alone (no tensor, no launch; the module switches are read now).  widths: the layers'
    output channels; xyz_grad / feat_grad: a gradient flows into the coordinates / the features; plan_gs, plan_unit_map: group
    size of the plan that came with idx (None: none did) and whether it carries a unit map; no_grad: nothing will ask this
    pass for a backward (eval under torch.no_grad(): the forward may keep nothing)."""
    L, P = len(widths), B * M * S
    if not training:
        if no_grad and EVAL_CHAIN and eval_chain_ok(S, _round_up(_round_up(cin_raw, 8) + 3, 32), widths):
            return StageRoute(False, "chain", 0, False, ("lds",) * (L - 1), ("folded",) * L, "", "y", False)
        return StageRoute(False, "grouped", 0, False, ("stored",) * (L - 1), ("running",) * L, "", "y", False)
    xgen = not has_features and xyzgen_ok(P, L, widths[0], xyz_grad) and affine_pays(P, widths[1])
    plan, arrives = None, False
    if row_plan_ok(True, S, P, L, xyz_grad or (feat_grad and N > 8192), 128 % S == 0):
        arrives = plan_gs == PLAN_GROUP
        plan = _Plan()                        # what the predicates below ask of the plan forward will use
        plan.gs, plan.unit_src = PLAN_GROUP, (True if (plan_unit_map or not arrives) else None)
    hoist = hoist_ok(True, has_features or None, _round_up(cin_raw, 8), cin_raw, L, widths[0], xgen)
    feed = tuple("yab" if (affine_pays(P, widths[l + 1]) or (xgen and l == 0)) else "stored" for l in range(L - 1))
    extrema = bool(POOL_EPILOGUE) and 128 % S == 0
    no_dy = extrema and L >= 2 and feed[-1] == "yab" and last_no_dy_ok(plan, L, P, widths[-2], widths[-1], S, True)
    return StageRoute(
        True, "xyz" if xgen else "source" if hoist else "grouped", plan.gs if plan is not None else 0, arrives, feed,
        tuple("consumer" if f == "yab" else "relu" for f in feed) + ("pool" if extrema and widths[-1] <= 1024 else "launch",),
        "" if not extrema else "one" if (plan is not None and plan.gs == 8 and ONE_SIDED_EXTREMA) else "both",
        "no_dy" if no_dy else "ysel" if extrema else "y", bool(no_dy and LAST_X2))


def _count_uses(route):
    """the counters the tests read to see which route ran"""
    global xyzgen_uses, row_plan_uses, hoist_uses, last_no_dy_uses, eval_chain_uses
    eval_chain_uses += route.first == "chain"
    xyzgen_uses += route.first == "xyz"
    hoist_uses += route.first == "source"
    row_plan_uses += route.plan_gs > 0
    last_no_dy_uses += route.last == "no_dy"


# ---- forward steps: each allocates its buffers and makes its calls (inside the caller's _row_plan block) ----

def _new_layer(l, W, g, training):
    """Layer l with its prepared weight.  The reference concatenates [xyz(3), features(cin)] (pointnet2_utils.py:357-359); the
    gathered rows are [features(cin), xyz(3), 0-pad] so that feature pieces stay 16-byte aligned -- layer 0 rotates the weight
    columns to match."""
    lay = _Layer()
    lay.X = lay.fin = None
    W2 = W.detach().reshape(W.shape[0], -1)
    padded_w = l == 0 and g.cin != g.cin_raw
    if padded_w:
        W2 = torch.nn.functional.pad(W2, (0, g.cin - g.cin_raw))     # zero columns for the padded feature channels
    lay.K, lay.C = (g.kpad if l == 0 else W2.shape[1]), W2.shape[0]
    lay.Wp, lay.Wt = prep_weight(W2, lay.C, lay.K, rot=3 if l == 0 else 0, transpose=training,
                                 persistent=is_persistent(W) and not padded_w)
    return lay


def _gather_rows(g, xyz_c, cen_c, idx, feat_pm, xpad, dev):
    """the grouped rows [features | xyz | 0-pad] (xpad = 8: the coordinates only, 16 bytes per grouped position); with a plan
    the gather writes the compact row space, and every later launch works on the rows in use"""
    X0 = torch.empty((g.P, xpad), device=dev, dtype=E16.dtype)
    _call(_lib.omnipq_sa_gather, xyz_c, g.B, g.N, g.M, g.S, g.cin, xpad, g.inv_r, _p(xyz_c), _p(cen_c), _p(idx), _p(feat_pm),
          _p(X0))
    return X0


def _first_generated(g, lay, X0, sums, dev):
    """first layer "xyz": never materialised (see XYZGEN), its statistics from the moments of the grouped coordinates"""
    lay.mom = torch.empty((12,), device=dev, dtype=torch.float64)
    _call(_lib.omnipq_sa_xyz_moments, X0, g.P, _p(X0), X0.shape[1], _p(lay.mom))
    _call(_lib.omnipq_sa_xyz_stats, X0, lay.C, _p(lay.Wp), lay.K, _p(lay.mom), _p(sums))
    lay.Y = None


def _first_on_source(g, lay, plan, xyz_c, cen_c, idx, feat2d, sums, dev):
    """first layer "source" (see HOIST_L1): Z = features W_f^T per source point, then Y = Z[idx] + W_x . xrel per grouped row
    with its statistics.  -> the rows' relative coordinates (the weight gradient's operand)"""
    B, N, M, S, P, cin = g[:6]
    Z = gemm_nt_f32(feat2d, lay.Wp, B * N, lay.C, cin, cin, lay.K)       # W_f = the first cin prepared columns
    lay.Y = torch.empty((P, lay.C), device=dev, dtype=E16.dtype)
    Xrel = torch.empty((P, 8), device=dev, dtype=E16.dtype)
    nws = int(_lib.omnipq_sa_l1_rows_workspace_bytes(B, M, S, lay.C))
    ws = torch.empty((nws // 4,), device=dev, dtype=torch.float32)
    tk = zeros_f32(nws // (8 * lay.C * 16) + 1, dev)                     # one zero word per 16 workgroups
    _call(_lib.omnipq_sa_l1_rows, Z, B, N, M, S, lay.C, g.inv_r, _p(xyz_c), _p(cen_c), _p(idx), _p(Z),
          ctypes.c_void_p(lay.Wp.data_ptr() + cin * lay.Wp.element_size()), lay.K,
          _p(plan.rows_dev if plan is not None else None), _p(plan.unit_src if plan is not None else None),
          _p(plan.row_w if plan is not None else None), _p(lay.Y), _p(Xrel), _p(sums), _p(ws), _p(tk))
    return Xrel


def _middle_layer(route, g, l, lay, below, X, X0, sums):
    if l == 1 and route.first == "xyz":
        lay.Y = gemm_nt_xyz(X0, below, lay.Wp, g.P, lay.C, lay.K, sums)
    elif route.feed[l - 1] == "yab":
        # the layer below never stored relu(bn(Y)): this GEMM rebuilds it while staging its operand
        lay.Y = gemm_nt_affine(below.Y, below, lay.Wp, g.P, lay.C, lay.K, sums=sums)
    else:
        lay.Y = _gemm_nt_stats(X, lay.Wp, g.P, lay.C, lay.K, sums)


def _last_layer(route, g, lay, below, X, sums, dev):
    """The last GEMM; route.extrema: it also records every ball's extrema, so the pooling pass needs no Y (a planned stage
    records them per group of the compact row space; pool_select merges a ball's).  -> its BallExtrema or None"""
    pool = None
    if route.extrema:
        per = route.plan_gs or g.S
        ext16 = torch.empty((2, g.P // per, lay.C), device=dev, dtype=E16.dtype)
        ext8 = torch.empty((2, g.P // per, lay.C), device=dev, dtype=torch.uint8)
        pool = BallExtrema(per, ext16[0], ext16[1], ext8[0], ext8[1])
    if below is not None and route.feed[-1] == "yab":
        lay.Y = gemm_nt_affine(below.Y, below, lay.Wp, g.P, lay.C, lay.K, sums=sums, pool=pool, store=route.last != "no_dy")
    else:
        lay.Y = _gemm_nt_stats(X, lay.Wp, g.P, lay.C, lay.K, sums, pool=pool)
    return pool


# The BatchNorm finalise steps of a layer `lay` (a _Layer here, a rows_mlp._L), for the SA stage and the rows engine alike.
# bn: running_mean, running_var, momentum, eps (a StageBN, a rows_mlp.Layer); conv_bias: the bias of the linear layer in front
def batch_constants(lay, sums, count, gamma, beta, bn, conv_bias=None):
    """training: the (4, C) buffer a | b | mean | invstd and its four views on `lay` -> the Finalize of the launch that fills
    them: the layer's own (finalize_launch) or its first consumer's (lay.fin: gemm_nt_affine / _xyz, _pool_forward)"""
    stats = torch.empty((4, lay.C), device=sums.device)
    lay.a, lay.b, lay.mean, lay.invstd = stats[0], stats[1], stats[2], stats[3]
    return Finalize(sums, count, gamma.detach(), beta.detach(), bn.eps, bn.momentum, bn.running_mean, bn.running_var,
                    None if conv_bias is None else conv_bias.detach().float().contiguous())


def finalize_launch(lay, rows, fin, relu):
    """the layer's own launch: constants and running-statistics update; relu: with the normalise + ReLU pass.  -> lay.X"""
    if relu:
        lay.X = torch.empty_like(lay.Y)
        _call(_lib.omnipq_bn_finalize_relu, lay.Y, rows, lay.C, fin.count, _p(fin.sums), *fin.tail(), _p(fin.conv_bias),
              _p(lay.Y), _p(lay.X), _p(lay.a), _p(lay.b), _p(lay.mean), _p(lay.invstd))
    else:
        _call(_lib.omnipq_bn_finalize, fin.sums, lay.C, fin.count, _p(fin.sums), *fin.tail(), _p(lay.a), _p(lay.b), _p(lay.mean),
              _p(lay.invstd), _p(fin.conv_bias))
    return lay.X


def running_constants(lay, rows, gamma, beta, bn, conv_bias=None, relu=True):
    """eval mode: constants from the running estimates (the bias only shifts the mean); relu: then the normalise + ReLU pass
    (the last layer of an SA stage leaves it to the pool).  -> lay.X"""
    lay.invstd = torch.rsqrt(bn.running_var + bn.eps)
    lay.mean = bn.running_mean - conv_bias.detach().float() if conv_bias is not None else bn.running_mean
    lay.a = (gamma.detach() * lay.invstd).contiguous()
    lay.b = (beta.detach() - lay.mean * lay.a).contiguous()
    if relu:
        lay.X = torch.empty_like(lay.Y)
        _call(_lib.omnipq_bnrelu, lay.Y, rows, lay.C, _p(lay.Y), _p(lay.a), _p(lay.b), _p(lay.X))
    return lay.X


def _batch_norm(how, g, lay, sums, gamma, beta, bn):
    """a training layer's statistics exchange, its finalise where the route puts it (StageRoute.finalize), its step counter"""
    _allreduce_(sums, g.world)
    fin = batch_constants(lay, sums, float(g.P) * g.world, gamma, beta, bn)
    if how in ("consumer", "pool"):
        lay.fin = fin
    else:
        finalize_launch(lay, g.P, fin, relu=how == "relu")
    bump(bn.num_batches_tracked)
    return lay.X


def _eval_chain(route, g, plan, xyz_c, cen_c, idx, feat_pm, params, bn, dev):
    """route "chain" (see EVAL_CHAIN): the whole stage as ONE launch.  -> what _forward_layers returns: no stored rows, pooled
    inside the launch, and no arg-max -- there is no backward"""
    L = len(bn)
    layers = [_new_layer(l, params[3 * l], g, False) for l in range(L)]
    recs = (_InferLayer * L)()
    keep = []                                   # the f32 vectors the records point to (copies, where a buffer is not f32)
    for l, (lay, rec) in enumerate(zip(layers, recs)):
        vecs = [v.detach().float().contiguous() for v in (*params[3 * l + 1:3 * l + 3], bn[l].running_mean, bn[l].running_var)]
        keep.append(vecs)
        rec.W, rec.ldw, rec.C = lay.Wp.data_ptr(), lay.Wp.stride(0), lay.C
        rec.gamma, rec.beta, rec.running_mean, rec.running_var = (v.data_ptr() for v in vecs)
        rec.eps = bn[l].eps
    C = layers[-1].C
    out_f32 = torch.empty((g.B, g.M, C), device=dev, dtype=torch.float32)
    out_pm = torch.empty((g.B * g.M, C), device=dev, dtype=E16.dtype)
    _call(_lib.omnipq_sa_infer, xyz_c, g.B, g.N, g.M, g.S, g.cin, g.kpad, g.inv_r, _p(xyz_c), _p(cen_c), _p(idx), _p(feat_pm), L,
          ctypes.byref(recs), _p(out_f32), _p(out_pm))
    return layers, None, None, (out_f32, out_pm, None, None)


def _forward_layers(route, g, plan, xyz_c, cen_c, idx, feat_pm, params, bn, dev):
    """every route but "chain": layer by layer, then the pool.  -> (layers, X0, the relative coordinates of a "source" first
    layer, what _pool_forward returns)"""
    L = len(bn)
    layers, Xrel, pooled = [], None, None
    xpad = 8 if route.first == "xyz" else g.kpad
    X = X0 = None if route.first == "source" else _gather_rows(g, xyz_c, cen_c, idx, feat_pm, xpad, dev)
    for l in range(L):
        W, gamma, beta = params[3 * l:3 * l + 3]
        lay = _new_layer(l, W, g, route.training)
        sums = zeros_f64(2, lay.C, dev) if route.training else None
        if not route.training:
            lay.Y = _gemm_nt(X, lay.Wp, g.P, lay.C, lay.K)         # eval mode: every activation stored, the last one for the pool
            X = running_constants(lay, g.P, gamma, beta, bn[l], relu=l < L - 1)
        elif l == L - 1:
            # route.extrema "one": for the last GEMM and the pool-select launch the plan names the gamma whose sign selects
            with _row_plan(plan, g.P, pool_gamma=gamma.detach() if route.extrema == "one" else None):
                pool = _last_layer(route, g, lay, layers[-1] if l else None, X, sums, dev)
                _batch_norm(route.finalize[l], g, lay, sums, gamma, beta, bn[l])
                pooled = _pool_forward(route, g, lay, pool, dev)
        else:
            if l > 0:
                _middle_layer(route, g, l, lay, layers[-1], X, X0, sums)
            elif route.first == "xyz":
                _first_generated(g, lay, X0, sums, dev)
            elif route.first == "source":
                Xrel = _first_on_source(g, lay, plan, xyz_c, cen_c, idx, feat_pm.reshape(g.B * g.N, g.cin), sums, dev)
            else:
                lay.Y = _gemm_nt_stats(X0, lay.Wp, g.P, lay.C, lay.K, sums)   # first layer "grouped": GEMM + batch statistics
            X = _batch_norm(route.finalize[l], g, lay, sums, gamma, beta, bn[l])
        layers.append(lay)
    return layers, X0, Xrel, pooled or _pool_forward(route, g, layers[-1], None, dev)      # (eval mode: the pool scans Y)


def _pool_forward(route, g, last, pool, dev):
    """max-pool over every ball -> (out f32 [B][M][C], its 16-bit twin, the arg-max rows, the selected pre-BN values | None)"""
    B, M, S = g.B, g.M, g.S
    out_f32 = torch.empty((B, M, last.C), device=dev, dtype=torch.float32)
    out_pm = torch.empty((B * M, last.C), device=dev, dtype=E16.dtype)
    arg = torch.empty((B * M, last.C), device=dev, dtype=torch.uint8)
    if not route.extrema:
        _call(_lib.omnipq_sa_pool, last.Y, B, M, S, last.C, _p(last.Y), _p(last.a), _p(last.b), _p(out_f32), _p(out_pm), _p(arg))
        return out_f32, out_pm, arg, None
    ysel = torch.empty((B * M, last.C), device=dev, dtype=E16.dtype)
    if route.finalize[-1] == "pool":
        last.fin, fin = None, last.fin                # the first consumer finalises
        _call(_lib.omnipq_sa_pool_select_finalize, out_pm, B * M, last.C, *pool.args(), _p(fin.sums), fin.count, *fin.tail(),
              _p(last.a), _p(last.b), _p(last.mean), _p(last.invstd), _p(out_f32), _p(out_pm), _p(arg), _p(ysel))
    else:
        _call(_lib.omnipq_sa_pool_select, out_pm, B * M, last.C, *pool.args(), _p(last.a), _p(last.b), _p(out_f32), _p(out_pm),
              _p(arg), _p(ysel))
    return out_f32, out_pm, arg, ysel


# ---- backward steps: ctx is the stage's saved state; the other arguments are what this backward pass has computed so far ----

def _exchanges(world):
    """the BatchNorm-backward totals are summed over ranks between the statistics and the apply launch"""
    return world > 1 or _FORCE_COLLECTIVES


def _pool_bwd_apply(ctx, g_out, sums, grads):
    """routes "y" / "ysel": dY of the last layer from the pool's gradient and the totals `sums`, and its affine gradients
    (dgamma = sum dz * yhat, dbeta = sum dz: LOCAL totals -- DDP averages them -- taken before the all-reduce)"""
    g, last, i = ctx.geom, ctx.layers[-1], 3 * (len(ctx.layers) - 1)
    dY = torch.empty_like(last.Y)
    if _exchanges(g.world):
        grads[i + 1], grads[i + 2] = affine_grads(sums, last.C)
        _allreduce_(sums[:2], g.world)
        _call(_lib.omnipq_sa_pool_bwd_apply, g_out, g.B, g.M, g.S, last.C, float(g.P) * g.world, _p(last.Y), _p(last.a),
              _p(last.mean), _p(last.invstd), _p(sums), _p(g_out), _p(ctx.out_pm), _p(ctx.arg), _p(dY))
    else:
        gb3 = torch.empty((2, last.C), device=dY.device, dtype=torch.float32)      # dbeta | dgamma, written by the apply
        grads[i + 1], grads[i + 2] = gb3[1], gb3[0]
        _call(_lib.omnipq_sa_pool_bwd_apply_gb, g_out, g.B, g.M, g.S, last.C, float(g.P) * g.world, _p(last.Y), _p(last.a),
              _p(last.mean), _p(last.invstd), _p(sums), _p(g_out), _p(ctx.out_pm), _p(ctx.arg), _p(dY), _p(gb3))
    return dY, None


def _last_bwd_from_y(ctx, g_out, grads, dfr):
    g, last = ctx.geom, ctx.layers[-1]
    sums = torch.empty((3, last.C), device=g_out.device, dtype=torch.float64)
    _call(_lib.omnipq_sa_pool_bwd_stats, g_out, g.B, g.M, g.S, last.C, _p(last.Y), _p(last.mean), _p(last.invstd), _p(g_out),
          _p(ctx.out_pm), _p(ctx.arg), _p(sums))
    return _pool_bwd_apply(ctx, g_out, sums, grads)


def _last_bwd_from_ysel(ctx, g_out, grads, dfr):
    g, last = ctx.geom, ctx.layers[-1]
    sums = zeros_f64(3, last.C, g_out.device)                                   # [S | T | scratch], zero from the arena
    _call(_lib.omnipq_sa_pool_bwd_stats_sel, g_out, g.B * g.M, last.C, _p(ctx.ysel), _p(last.mean), _p(last.invstd), _p(g_out),
          _p(ctx.out_pm), _p(sums), 1)
    return _pool_bwd_apply(ctx, g_out, sums, grads)


def _last_bwd_no_dy(ctx, g_out, grads, dfr):
    """route "no_dy" (see LAST_NO_DY).  -> (dX2, the BatchNorm-backward totals of the layer below)"""
    g, plan, dev = ctx.geom, ctx.plan, g_out.device
    B, M, S, P, world = g.B, g.M, g.S, g.P, g.world
    L = len(ctx.layers)
    last, below = ctx.layers[-1], ctx.layers[-2]
    C3, C2 = last.C, last.K
    # the statistics pass also leaves the one-hot operand, from the values it reads anyway
    sums = zeros_f64(3, C3, dev)
    hot = torch.empty((B * M, C3), device=dev, dtype=torch.int32)
    _call(_lib.omnipq_sa_pool_bwd_stats_sel_hot, g_out, B * M, C3, _p(ctx.ysel), _p(last.mean), _p(last.invstd), _p(g_out),
          _p(ctx.out_pm), _p(sums), 1, _p(last.a), _p(ctx.arg), _p(hot))
    gb3 = None
    if _exchanges(world):
        grads[3 * (L - 1) + 1], grads[3 * (L - 1) + 2] = affine_grads(sums, C3)
        _allreduce_(sums[:2], world)
    else:
        gb3 = torch.empty((2, C3), device=dev, dtype=torch.float32)      # dbeta | dgamma, written by the prep
        grads[3 * (L - 1) + 1], grads[3 * (L - 1) + 2] = gb3[1], gb3[0]
    B1 = torch.empty((C2, C2 + 32), device=dev, dtype=E16.dtype)
    ab = torch.empty((2, C3), device=dev, dtype=torch.float32)          # alpha | beta
    _call(_lib.omnipq_sa_last_bwd_prep, g_out, B * M, C3, C2, _p(sums), float(P) * world, _p(last.a), _p(last.mean),
          _p(last.invstd), _p(None), _p(None), _p(None), _p(last.Wt), last.Wt.stride(0), _p(None), _p(B1), C2 + 32, _p(ab[0]),
          _p(ab[1]), _p(gb3))
    # the data gradient + the BatchNorm-backward sums of the layer below; X2 = relu(bn2(Y2)) as its first phase forms
    # it is kept for the weight gradient (LAST_X2: the TN launch is bound by rebuilding X2 in every fragment)
    want_w = ctx.needs_input_grad[_PARAMS_AT + 3 * (L - 1)]
    X2 = torch.empty((P, C2), device=dev, dtype=E16.dtype) if (want_w and ctx.route.keep_x2) else None
    pend = zeros_f64(3, below.C, dev)
    dX2 = torch.empty((P, C2), device=dev, dtype=E16.dtype)
    ws = _stats_workspace(P, C2, dev)
    _call(_lib.omnipq_gemm_nt_e16_dz_bnbwd, dX2, P, C2, C3, _p(below.Y), C2, _p(B1), C2 + 32, _p(last.Wt), last.Wt.stride(0),
          _p(hot), _p(plan.unit_src), S, _p(dX2), C2, _p(below.a), _p(below.b), _p(below.mean), _p(below.invstd), _p(pend),
          _p(ws), _p(X2))
    # the layer's weight gradient: from X2 (or Y2) and `hot`, with the other SA stages' when the deferred block ends
    if want_w:
        wt = ctx.wtargets[L - 1] if (dfr is not None and SA_WGRADS_GROUPED) else None
        src, blw = (X2, None) if X2 is not None else (below.Y, below)
        if wt is not None and wt.covers(C3 * C2):
            dfr.add_dz((src, blw, hot, plan, S, C3, C2, P, ab[0], ab[1], last.Wp), wt, ctx.stage_label)
        else:
            grads[3 * (L - 1)] = last_wgrad_dz(src, blw, hot, plan, S, C3, C2, P, ab[0], ab[1], last.Wp).view(C3, C2, 1, 1)
    return dX2, pend


_LAST_BWD = {"y": _last_bwd_from_y, "ysel": _last_bwd_from_ysel, "no_dy": _last_bwd_no_dy}


def _layer_wgrad(ctx, l, dY, grads, dfr):
    """the weight gradient of layer l (not a "source" first layer) from dY = the gradient w.r.t. its pre-BN output: collected
    for the grouped launch of ALL SA stages when the deferred_wgrads block ends, or launched now"""
    g, lay = ctx.geom, ctx.layers[l]
    below = ctx.layers[l - 1] if (l > 0 and ctx.route.feed[l - 1] == "yab") else None
    Xin = below.Y if below is not None else (ctx.layers[l - 1].X if l > 0 else ctx.X0)
    wt = ctx.wtargets[l] if (dfr is not None and SA_WGRADS_GROUPED) else None
    if wt is not None and ctx.needs_input_grad[_PARAMS_AT + 3 * l]:
        if l == 0:
            dfr.add_sa(dY, Xin, lay.C, lay.K, g.P, wt, Crop(lay.C, g.cin_raw + 3, rot=3 | (g.cin << 8)), blk=ctx.plan)
        else:
            dfr.add_sa(dY, Xin, lay.C, lay.K, g.P, wt, Crop(lay.C, lay.K), below, blk=ctx.plan)
        return
    dWp = _gemm_tn(dY, Xin, lay.C, lay.K, g.P, below=below)      # [Cout][K]
    wk = g.cin + 3 if l == 0 else lay.K
    grads[3 * l] = unprep_wgrad(dWp, lay.C, wk, 3 if l == 0 else 0, (lay.C, wk, 1, 1))
    if l == 0 and g.cin_raw != g.cin:
        grads[0] = grads[0][:, :g.cin_raw + 3].contiguous()       # drop the padded feature columns


def _layer_bwd(ctx, l, dY, grads, dfr):
    """layer l > 0.  -> (the gradient w.r.t. the ReLU output of the layer below, that layer's BatchNorm-backward totals)"""
    lay, prev = ctx.layers[l], ctx.layers[l - 1]
    _layer_wgrad(ctx, l, dY, grads, dfr)
    pend = zeros_f64(3, prev.C, dY.device)
    # Wt = [K][Cout]; the BN-backward sums of the layer below come out of the same pass
    return _gemm_nt_bnbwd(dY, lay.Wt, ctx.geom.P, lay.K, lay.C, prev, pend), pend


def _tail_grouped(ctx, dY, grads, dfr):
    """first layer "grouped": its weight gradient, then the rows' gradient summed per source point.  -> (d_xyz, d_cen, d_feat)"""
    B, N, M, S, P, cin, cin_raw, kpad, inv_r, _ = ctx.geom
    lay, dev = ctx.layers[0], dY.device
    _layer_wgrad(ctx, 0, dY, grads, dfr)
    want_xyz = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    want_feat = ctx.has_features and ctx.needs_input_grad[2]
    d_xyz = d_cen = d_feat = None
    if not (want_xyz or want_feat):
        return d_xyz, d_cen, d_feat
    dX = _gemm_nt(dY, lay.Wt, P, lay.K, lay.C)
    dfeat_pm = torch.empty((B, N, cin), device=dev) if want_feat else None
    if want_xyz:
        d_xyz = torch.empty((B, N, 3), device=dev)
        d_cen = torch.empty((B, M, 3), device=dev)
    # bucket the positions by source point, then every (point, 8-channel piece) sums its
    # own bucket: no atomics, each dX row is read exactly once
    offsets, order = _csr_of(ctx.csr_ahead, ctx.idx, B, N, M, S, ctx.plan, dX)
    _call(_lib.omnipq_sa_scatter_csr, dX, B, N, M, S, cin, kpad, inv_r, _p(offsets), _p(order), _p(dX), _p(dfeat_pm), _p(d_xyz),
          _p(d_cen))
    if dfeat_pm is not None:
        d_feat = dfeat_pm[..., :cin_raw].transpose(1, 2).to(ctx.feat_dtype)      # (B, cin, N) view, see forward
    return d_xyz, d_cen, d_feat


def _tail_generated(ctx, dY, grads):
    """first layer "xyz", reached at layer 1 (dY = the gradient w.r.t. ITS pre-BN output): layer 1's weight gradient contracts
    against activations rebuilt from the grouped coordinates, and its data-gradient GEMM is reduced to the five column sums
    the first layer's dW / dgamma / dbeta follow from"""
    P, world, dev = ctx.geom.P, ctx.geom.world, dY.device
    prev, lay, X0c = ctx.layers[0], ctx.layers[1], ctx.X0
    dWp = torch.empty((lay.C, lay.K), device=dev, dtype=torch.float32)
    ws = torch.empty((int(_lib.omnipq_gemm_tn_workspace_floats(lay.C, lay.K, P)),), device=dev, dtype=torch.float32)
    _call(_lib.omnipq_gemm_tn_e16_xyz_affine, dY, lay.C, lay.K, P, _p(dY), lay.C, _p(X0c), X0c.shape[1], _p(prev.Wp),
          prev.Wp.shape[1], _p(prev.a), _p(prev.b), _p(dWp), _p(ws))
    grads[3] = unprep_wgrad(dWp, lay.C, lay.K, 0, (lay.C, lay.K, 1, 1))
    sums5 = zeros_f64(5, prev.C, dev)
    ws5 = torch.empty((int(_lib.omnipq_gemm_nt_xyz_workspace_floats(P, prev.C)),), device=dev, dtype=torch.float32)
    _call(_lib.omnipq_gemm_nt_e16_xyz_bnbwd, dY, P, prev.C, lay.C, _p(dY), lay.C, _p(lay.Wt), lay.C, _p(X0c), X0c.shape[1],
          _p(prev.Wp), prev.Wp.shape[1], _p(prev.a), _p(prev.b), _p(prev.mean), _p(prev.invstd), _p(sums5), _p(ws5))
    grads[1], grads[2] = affine_grads(sums5, prev.C)            # this rank's dgamma / dbeta
    _allreduce_(sums5[:2], world)
    dW0 = torch.empty((prev.C, 3, 1, 1), device=dev, dtype=torch.float32)
    _call(_lib.omnipq_sa_xyz_bwd, dY, prev.C, _p(prev.Wp), prev.Wp.shape[1], _p(prev.mom), _p(sums5), _p(prev.a), _p(prev.mean),
          _p(prev.invstd), 1.0 / (float(P) * world), _p(dW0))
    grads[0] = dW0


def _tail_on_source(ctx, dY, grads, dfr):
    """first layer "source" (HOIST_L1): dY = the gradient w.r.t. its pre-BatchNorm output, (rows, C1) 16-bit.  Per-point sums
    of dY's rows first (CSR, no atomics), then everything is a contraction over the B * N points: dW_f = dZ^T features,
    d features = dZ W_f; the three coordinate columns of the weight take dW_x = dY^T xrel over the rows.
    -> (d_xyz, d_cen, d_feat)"""
    B, N, M, S, P, cin, cin_raw, _, inv_r, _ = ctx.geom
    feat2d, Xrel = ctx.hoist
    plan, lay, dev = ctx.plan, ctx.layers[0], dY.device
    C1 = lay.C
    want_xyz = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    want_feat = ctx.has_features and ctx.needs_input_grad[2]
    want_w = ctx.needs_input_grad[_PARAMS_AT]
    d_xyz = d_cen = d_feat = None
    if not (want_xyz or want_feat or want_w):
        return d_xyz, d_cen, d_feat
    offsets, order = _csr_of(ctx.csr_ahead, ctx.idx, B, N, M, S, plan, dY)
    dXr = None
    if want_xyz:
        # gradient of the relative coordinates: dY W_x (the rows cin .. cin + 7 of the transposed prepared weight: W_x^T | 0)
        dXr = torch.empty((P, 8), device=dev, dtype=E16.dtype)
        _call(_lib.omnipq_gemm_nt_e16, dY, P, 8, C1, _p(dY), C1,
              ctypes.c_void_p(lay.Wt.data_ptr() + cin * C1 * lay.Wt.element_size()), C1, _p(dXr), 8)
        d_xyz = torch.empty((B, N, 3), device=dev)
        d_cen = torch.empty((B, M, 3), device=dev)
    dZ = torch.empty((B * N, C1), device=dev, dtype=E16.dtype)
    _call(_lib.omnipq_sa_scatter_rows_csr, dY, B, N, M, S, C1, inv_r, _p(offsets), _p(order), _p(dY), _p(dXr),
          _p(plan.goff if plan is not None else None), plan.gs if plan is not None else 16, _p(None), _p(dZ), _p(d_xyz),
          _p(d_cen))
    if want_w:
        wt = ctx.wtargets[0] if (dfr is not None and SA_WGRADS_GROUPED) else None
        ld = cin_raw + 3
        if wt is not None:
            # the parameter's columns are [xyz(3) | features(cin)] (pointnet2_utils.py:357-359): two problems of the grouped
            # launch write the two column ranges of one gradient buffer
            dfr.add_sa(dZ, feat2d, C1, cin, B * N, wt, Crop(C1, cin, col0=3, ld=ld))
            dfr.add_sa(dY, Xrel, C1, 8, P, wt, Crop(C1, 3, col0=0, ld=ld), blk=plan)
        else:
            dWf = _gemm_tn(dZ, feat2d, C1, cin, B * N)
            dWx = _gemm_tn(dY, Xrel, C1, 8, P)              # (inside backward()'s _row_plan block: the rows in use)
            grads[0] = torch.cat([dWx[:, :3], dWf], 1).view(C1, ld, 1, 1)
    if want_feat:
        # d features = dZ W_f: the first cin rows of the transposed prepared weight are W_f^T, K-contiguous over C1
        dfeat = gemm_nt_f32(dZ, lay.Wt, B * N, cin, C1, C1, C1)
        d_feat = dfeat.view(B, N, cin).transpose(1, 2).to(ctx.feat_dtype)
    return d_xyz, d_cen, d_feat


# a layer's BatchNorm state as the stage uses it: the module's own buffers, and its two numbers
StageBN = collections.namedtuple("StageBN", "running_mean running_var num_batches_tracked momentum eps")


class StageCall(typing.NamedTuple):
    """What run() knows of a stage pass and the tensors do not say: ONE argument of FusedSAStage.apply."""
    label: str             # the stage's name for the timing sink, forward and backward ("sa1" .. "vote", or m<npoint>s<nsample>)
    radius: float
    normalize_xyz: bool
    training: bool
    sync: bool             # do the stage's BatchNorm layers exchange their statistics across ranks (SyncBatchNorm)?
    no_grad: bool          # autograd was off at the call: asked by apply's caller, inside a Function's forward it is always off
    bn: tuple              # a StageBN per layer
    plan: typing.Any       # the stage's _Plan and the chain_plan.Csr of its backward where they were made ahead of the stage
    csr: typing.Any        # (run(group=)), else None


def stage_call(module, grad_enabled, plan=None, csr=None):
    """The StageCall of a PointnetSAModuleVotes (no launch, no tensor made)."""
    bns = [_bn_of(layer)[1] for layer in module.mlp_module]
    return StageCall(getattr(module, "omnipq_stage", None) or f"m{module.npoint}s{module.nsample}", float(module.radius),
                     bool(module.normalize_xyz), bool(module.training), all(bool(bn_syncs(bn)) for bn in bns), not grad_enabled,
                     tuple(StageBN(bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.momentum), float(bn.eps))
                           for bn in bns), plan, csr)


_PARAMS_AT = 6          # FusedSAStage.apply: its arguments in front of *params


class FusedSAStage(torch.autograd.Function):
    """forward(xyz, new_xyz, features|None, feat_pm|None, idx, call, *params) -> (B, C_last, M) f32 and its 16-bit
    position-major twin.  call: the pass's StageCall; params = (W_0, gamma_0, beta_0, W_1, ...)."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, features, feat_pm, idx, call, *params):
        ctx.e16 = E16.dtype
        ctx.n_inputs = _PARAMS_AT + len(params)
        ctx.stage_label = call.label
        with _tagged("@sa", ctx.stage_label):
            return FusedSAStage._forward(ctx, xyz, new_xyz, features, feat_pm, idx, call, *params)

    @staticmethod
    def _forward(ctx, xyz, new_xyz, features, feat_pm, idx, call, *params):
        dev = xyz.device
        B, N, _ = xyz.shape
        M, S = idx.shape[1], idx.shape[2]
        L = len(params) // 3
        training, plan = call.training, call.plan
        cin_raw = 0 if features is None else features.shape[1]
        cin = _round_up(cin_raw, 8)
        g = _Geom(B, N, M, S, B * M * S, cin, cin_raw, _round_up(cin + 3, 32),
                  (1.0 / call.radius) if call.normalize_xyz else 1.0, _world() if (training and call.sync) else 1)
        route = stage_route(training, B, N, M, S, cin_raw, [params[3 * l].shape[0] for l in range(L)], features is not None,
                            ctx.needs_input_grad[0] or ctx.needs_input_grad[1],
                            features is not None and ctx.needs_input_grad[2], None if plan is None else plan.gs,
                            plan is not None and plan.unit_src is not None, no_grad=call.no_grad)
        _count_uses(route)
        if features is None:
            feat_pm = None
        elif feat_pm is None or cin != cin_raw:
            # position-major bf16 copy [B][N][cin] (a producer that has one passes it in: see run())
            feat_pm = features.detach().transpose(1, 2).to(E16.dtype)
            feat_pm = torch.nn.functional.pad(feat_pm, (0, cin - cin_raw)) if cin != cin_raw else feat_pm.contiguous()
        xyz_c = xyz.detach().contiguous()
        cen_c = new_xyz.detach().contiguous()
        if not route.plan_gs:
            plan = None
        elif not route.plan_arrives:
            plan = make_row_plan(idx, g.P)
        with _row_plan(plan, g.P):
            layers, X0, Xrel, (out_f32, out_pm, arg, ysel) = (_eval_chain if route.first == "chain" else _forward_layers)(
                route, g, plan, xyz_c, cen_c, idx, feat_pm, params, call.bn, dev)
        ctx.route, ctx.geom, ctx.plan = route, g, plan
        ctx.layers, ctx.X0 = layers, X0
        ctx.hoist = (feat_pm.reshape(B * N, cin), Xrel) if route.first == "source" else None
        # where a layer's weight gradient may be written behind autograd's back (deferred_wgrads): Parameters only
        ctx.wtargets = [grad_target(params[3 * l]) for l in range(L)] if training else None
        ctx.idx, ctx.csr_ahead = idx, call.csr
        ctx.out_pm, ctx.arg, ctx.ysel = out_pm, arg, ysel
        ctx.has_features = features is not None
        ctx.feat_dtype = features.dtype if features is not None else None
        ctx.training = training
        twin = out_pm.view(B, M, layers[-1].C)
        ctx.mark_non_differentiable(twin)
        ctx.set_materialize_grads(False)        # no zero tensor of the twin's size per backward (its gradient is never used)
        # reference layout (B, C, M) as a VIEW of the position-major result: values, shape and dtype are
        # the reference's, only the strides differ (no transpose pass; every consumer on this path
        # either accepts strides or wants the position-major form back)
        return out_f32.transpose(1, 2), twin

    @staticmethod
    def backward(ctx, g_out, _g_twin=None):
        E16.select(ctx.e16)
        if g_out is None:                       # the stage's output took no part in the loss
            return (None,) * ctx.n_inputs
        with _tagged("@sa", ctx.stage_label), _row_plan(ctx.plan, ctx.geom.P):
            return FusedSAStage._backward(ctx, g_out)

    @staticmethod
    def _backward(ctx, g_out):
        if not ctx.training:
            raise RuntimeError("FusedSAStage: backward in eval mode is not supported (use the composed path)")
        route, g, layers = ctx.route, ctx.geom, ctx.layers
        L = len(layers)
        g_out = g_out.float().transpose(1, 2).contiguous()      # position-major [B*M][C] (no-op for a view)
        grads = [None] * (3 * L)
        dfr = deferred_wgrads.active
        d_xyz = d_cen = d_feat = None
        # dY: the gradient w.r.t. layer l's pre-BN output -- or, while `pend` holds that layer's BatchNorm-backward totals,
        # still the gradient w.r.t. its ReLU output
        dY, pend = _LAST_BWD[route.last](ctx, g_out, grads, dfr)
        for l in range(L - 2 if route.last == "no_dy" else L - 1, -1, -1):
            if pend is not None:
                grads[3 * l + 1], grads[3 * l + 2] = bn_backward_apply(dY, layers[l], g.P, layers[l].C, float(g.P) * g.world,
                                                                       pend, g.world)
            if l == 1 and route.first == "xyz":
                _tail_generated(ctx, dY, grads)
                break
            if l == 0:
                d_xyz, d_cen, d_feat = (_tail_on_source if route.first == "source" else _tail_grouped)(ctx, dY, grads, dfr)
                break
            dY, pend = _layer_bwd(ctx, l, dY, grads, dfr)
        ctx.layers = None
        return (d_xyz, d_cen, d_feat) + (None,) * (_PARAMS_AT - 3) + tuple(grads)


def _bn_of(layer):
    """Conv2d wrapper (pytorch_utils._ConvBase) -> (conv, bn) or None if it is not conv+BN+ReLU."""
    conv = getattr(layer, "conv", None)
    bnw = getattr(layer, "bn", None)
    act = getattr(layer, "activation", None)
    if conv is None or bnw is None or not isinstance(act, torch.nn.ReLU):
        return None
    bn = getattr(bnw, "bn", None)
    if bn is None or conv.bias is not None or conv.kernel_size != (1, 1):
        return None
    if not isinstance(bn, (torch.nn.BatchNorm2d, torch.nn.SyncBatchNorm)):
        return None
    if bn.weight is None or bn.running_mean is None or bn.momentum is None:
        return None
    return conv, bn


def bn_syncs(bn):
    """Do the hand-written kernels have to all-reduce this layer's statistics?  Only for a SyncBatchNorm on the default
    process group (what nn.SyncBatchNorm.convert_sync_batchnorm produces, reference pq_transformer.py:194); a plain
    BatchNorm keeps per-rank statistics under DDP exactly as torch's does.  A custom process group is not supported by
    the kernels' collectives: None = use the composed path."""
    if not isinstance(bn, torch.nn.SyncBatchNorm):
        return False
    if getattr(bn, "process_group", None) is not None:
        return None
    return True


def eligible(module, xyz, features):
    """Can `module` (a PointnetSAModuleVotes) run its group+MLP+pool on the fused kernels?"""
    if not xyz.is_cuda or module.npoint is None or module.pooling != "max":
        return False
    grouper = module.grouper
    if getattr(grouper, "sample_uniformly", False) or not getattr(grouper, "use_xyz", True):
        return False
    if module.nsample > 255 or len(module.mlp_module) == 0:
        return False
    for layer in module.mlp_module:
        got = _bn_of(layer)
        if got is None:
            return False
        conv, bn = got
        # widths are contraction lengths of the data-gradient GEMM: multiples of the 32-wide K step
        if conv.out_channels % 32 or conv.out_channels > 640:
            return False
        if bn_syncs(bn) is None:
            return False
    if not module.training and torch.is_grad_enabled():
        return False
    return True


def run(module, xyz, new_xyz, features, group=None):
    """ball query + fused stage -> (B, C_out, npoint) f32.  group: a chain_plan.StageAhead -- the ball query (and row plan,
    and backward CSR with the row space it was built in) of this stage made ahead of it (they depend on coordinates only:
    Pointnet2Backbone's sampling chain)."""
    idx = plan = csr = None
    if group is not None and group.idx is not None and \
            tuple(group.idx.shape) == (xyz.shape[0], new_xyz.shape[1], module.nsample) and group.idx.dtype == torch.int32:
        idx, csr = group.idx, group.csr
        if group.plan_state is not None:
            B_, M_, S_ = idx.shape
            plan = plan_from_state(group.plan_state, B_, M_, B_ * M_ * S_)
    call = stage_call(module, torch.is_grad_enabled(), plan, csr)
    if idx is None:
        with _tagged("@sa", call.label):
            idx = pointnet2_utils.ball_query(module.radius, module.nsample, xyz, new_xyz)
    params = []
    for layer in module.mlp_module:
        conv, bn = _bn_of(layer)
        params += [conv.weight, bn.weight, bn.bias]
    feat_pm = None if features is None else rows16_of(features, (features.shape[0], features.shape[2], features.shape[1]))
    out, twin = FusedSAStage.apply(xyz, new_xyz, features, feat_pm, idx, call, *params)
    out.omnipq_rows16 = twin        # consumers that work on bf16 rows (next SA stage, FP modules) skip their cast
    return out


class FPGatherRows(torch.autograd.Function):
    """Input rows of a feature-propagation MLP, straight from position-major operands:
        rows[(b,i)] = [ sum_k w[b,i,k] * known_pm[b, idx[b,i,k], :]  |  skip_pm[b, i, :] ]        bf16 (B*n, C2 + C1)
    (reference pointnet2_modules.py:395-409: three_interpolate, cat along channels).  `known_feats` / `skip_feats`
    are the (B, C, .) tensors of the reference API -- they only carry the autograd edges; the arithmetic reads
    their bf16 twins.  Gradients come back in the (B, C, .) layout as views of position-major data."""

    @staticmethod
    def forward(ctx, known_feats, known_pm, skip_feats, skip_pm, idx, weight, csr):
        """csr: the chain_plan.Csr of the backward made ahead of the module (offsets (B, m+1), order (B, 3n)), or None"""
        ctx.e16 = E16.dtype
        B, n = idx.shape[0], idx.shape[1]
        m, C2 = known_pm.shape[1], known_pm.shape[2]
        C1 = 0 if skip_pm is None else skip_pm.shape[2]
        rows = torch.empty((B * n, C2 + C1), device=idx.device, dtype=E16.dtype)
        _call(_lib.omnipq_interp_rows, rows, B, n, m, C2, _p(known_pm), _p(idx), _p(weight), _p(rows), C2 + C1, 0)
        if C1:
            _call(_lib.omnipq_place_rows, rows, B * n, C1, _p(skip_pm), _p(rows), C2 + C1, C2)
        ctx.save_for_backward(idx, weight)
        ctx.pre_csr = csr
        ctx.geom = (B, n, m, C2, C1, known_feats.dtype, None if skip_feats is None else skip_feats.dtype)
        return rows

    @staticmethod
    def backward(ctx, g):
        E16.select(ctx.e16)
        idx, weight = ctx.saved_tensors
        B, n, m, C2, C1, kdt, sdt = ctx.geom
        g = g.to(E16.dtype).contiguous()
        d_known = d_skip = None
        if ctx.needs_input_grad[0]:
            # bucket the (unknown point, slot) pairs by the known point they read, then sum bucket-wise: no atomics
            dk = torch.empty((B, m, C2), device=g.device, dtype=torch.float32)
            pre = ctx.pre_csr
            if pre is not None and tuple(pre.offsets.shape) == (B, m + 1) and tuple(pre.order.shape) == (B, 3 * n):
                offsets, order = pre.offsets, pre.order
            else:
                offsets = torch.empty((B, m + 1), device=g.device, dtype=torch.int32)
                order = torch.empty((B, 3 * n), device=g.device, dtype=torch.int32)
                scratch = torch.empty((B, m), device=g.device, dtype=torch.int32)
                _call(_lib.omnipq_sa_build_csr, g, B, m, n, 3, _p(idx), _p(offsets), _p(order), _p(scratch))
            _call(_lib.omnipq_interp_rows_grad_csr, g, B, n, m, C2, _p(g), C2 + C1, 0, _p(offsets), _p(order), _p(weight),
                  _p(dk))
            d_known = dk.to(kdt).transpose(1, 2)
        if C1 and ctx.needs_input_grad[2]:
            d_skip = g.view(B, n, C2 + C1)[:, :, C2:].to(sdt).transpose(1, 2)
        return d_known, None, d_skip, None, None, None, None
