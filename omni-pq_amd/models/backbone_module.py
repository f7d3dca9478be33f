"""PointNet++ backbone: 4 set-abstraction + 2 feature-propagation layers
(reference models/backbone_module.py:21-139; layer hyper-parameters :38-75 are hard-coded there
and here).  Fills the `sa*_`, `fp2_` and `seed_` keys of `end_points`.
"""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT, os.path.join(_ROOT, "pointnet2")):
    if _p not in sys.path:
        sys.path.append(_p)

import weakref  # noqa: E402

from pointnet2_modules import PointnetSAModuleVotes, PointnetFPModule  # noqa: E402
import pointnet2_utils  # noqa: E402
import chain_plan  # noqa: E402
from chain_plan import Ahead, ChainPlan, ExtraLevel, Head, Pending, Tail  # noqa: E402

GROUP_AHEAD = True          # prefetched sampling chains also make the stages' centres / ball queries / row plans (see _launch_plan)

# (name, npoint, radius, nsample)
_SA_GEOMETRY = (("sa1", 2048, 0.2, 64), ("sa2", 1024, 0.4, 32), ("sa3", 512, 0.8, 16),
                ("sa4", 256, 1.2, 16))
_SA_NAMES = tuple(g[0] for g in _SA_GEOMETRY)
_FP_PAIRS = ((2, 3), (1, 2))        # (unknown stage, known stage) of fp1: sa3 <- sa4 and fp2: sa2 <- sa3

_STEP_STREAMS = []          # (weak reference to the owner, or None for a stream that lives as long as the process; stream)


def new_step_stream(device, owner=None, avoid=()):
    """A side stream for work that is forked off INSIDE a training step: the sampling chains here, the decoder's
    (decoder_rows._side_stream), a model's weight-gradient flushes (PQ_Transformer._flush_stream).  torch hands streams out of a
    pool of 32 per device, round-robin: a new Stream object can BE an earlier one.  That is harmless between two forks of one
    step -- except for a sampling stream: the plan of the first captured batch is launched BEFORE the capture and its events are
    waited for inside it, and once the same underlying stream has been pulled into the capture by another fork (the teacher's
    forward in front of the student's, say) or is the capture stream itself, that wait is refused
    (hipErrorStreamCaptureIsolation: the event's stream is capturing, the event is not part of the capture) and the capture is
    lost.  So every stream handed out here is none of `avoid`, not the stream torch captures graphs on, and none of the streams
    handed out earlier whose owner is still alive.  owner: the module the stream belongs to (held weakly)."""
    _STEP_STREAMS[:] = [(o, s) for o, s in _STEP_STREAMS if o is None or o() is not None]
    taken = {s.cuda_stream for _, s in _STEP_STREAMS}
    taken |= {s.cuda_stream for s in avoid if s is not None}
    cap = getattr(torch.cuda.graph, "default_capture_stream", None)
    if cap is not None:
        taken.add(cap.cuda_stream)
    stream = torch.cuda.Stream(device=device)
    for _ in range(64):
        if stream.cuda_stream not in taken:
            break
        stream = torch.cuda.Stream(device=device)
    _STEP_STREAMS.append((None if owner is None else weakref.ref(owner), stream))
    return stream


class Pointnet2Backbone(nn.Module):
    """input (B, N, 3 + input_feature_dim) -> 1024 seeds with 288-channel features."""

    def __init__(self, input_feature_dim=0, width=2, depth=2):
        super().__init__()
        self.depth = depth
        self.width = width
        hidden = [128 * width] * depth
        in_ch = [input_feature_dim, 128 * width, 256 * width, 256 * width]
        mid = [[64 * width] * depth, hidden, hidden, hidden]
        out_ch = [128 * width, 256 * width, 256 * width, 256 * width]
        for (name, npoint, radius, nsample), ci, cm, co in zip(_SA_GEOMETRY, in_ch, mid, out_ch):
            setattr(self, name, PointnetSAModuleVotes(npoint=npoint, radius=radius, nsample=nsample,
                                                      mlp=[ci] + cm + [co], use_xyz=True,
                                                      normalize_xyz=True))
        for name_ in _SA_NAMES:
            getattr(self, name_).omnipq_stage = name_      # label of the stage in per-stage timings (sa_fused.run)
        self.fp1 = PointnetFPModule(mlp=[256 * width + 256 * width, 256 * width, 256 * width])
        self.fp2 = PointnetFPModule(mlp=[256 * width + 256 * width, 256 * width, 288])

    # ---- sampling plan -----------------------------------------------------------------------
    # The four FPS passes of the backbone (and the one of FPSModule on the seeds) depend on the input
    # coordinates only, never on features: 40000 -> 2048 -> 1024 -> 512 -> 256 is a chain of
    # latency-bound kernels (thousands of dependent argmax rounds on a handful of CUs).  On a GPU
    # they run on a side stream: the sa1 pass can be started one batch ahead (`prefetch`), the
    # later ones overlap with the MLP of the previous layer.  Results are identical to calling
    # furthest_point_sample inside each SA layer (reference pointnet2_modules.py:233-236).
    _plan = None            # chain_plan.ChainPlan of the chain in flight
    _pending = None         # chain_plan.Pending: the chain that starts inside the next forward()
    _side = None
    _extra = None           # chain_plan.ExtraLevel of the batch just run through forward() (take_extra)
    # optional extra level of the plan: {"sa2": npoint} = also sample npoint of the sa2 centres (the model's
    # FPSModule on the seeds, pq_transformer.py:211-212, is such a coordinate-only sampling)
    plan_extra = None

    def __getstate__(self):
        # streams, events and the plan's index buffers are per-instance run-time state: copies and pickles of
        # the module (copy.deepcopy for an EMA teacher, torch.save of the whole model) start without them
        state = self.__dict__.copy()
        for k in ("_plan", "_side", "_plan_bufs", "_extra", "_pending", "_head_side", "_head", "_tail"):
            state.pop(k, None)
        return state

    def _new_stream(self, device, avoid=()):
        """A stream for a sampling chain that is neither one of `avoid`, nor a side stream another part of a step was given,
        nor the stream torch captures graphs on (new_step_stream)."""
        return new_step_stream(device, owner=self, avoid=avoid)

    def _side_stream(self, device):
        if self._side is None or self._side.device != device:
            self._side = self._new_stream(device, (self._head_side,))
        return self._side

    # ---- the sa1 level in two pieces ------------------------------------------------------------------------------------------
    # The sa1 level is 2047 of the chain's ~3800 dependent rounds.  Its rounds [0, k) -- the HEAD -- can run one step earlier than
    # the rest of the chain, on a second side stream (prefetch_head), into a persistent head state (temp, idx[:, :k]); once
    # that has been handed over (hand_over_head) a chain started with prefetch(..., resume=True) -- the TAIL -- continues the
    # level at round k instead of sampling from 0.  Everything behind sa1's picks is the same code.  Indices are identical:
    # _ext.furthest_point_sampling_resume continues a sampling from exactly that state.
    _head_side = None
    _head = None            # chain_plan.Head: the head in flight
    _tail = None            # chain_plan.Tail: the handed-over state the next resumed chain continues
    resumed_levels = 0      # sa1 levels that continued a head (launched or captured) -- for tests and A/B scripts

    def _head_stream(self, device):
        if self._head_side is None or self._head_side.device != device:
            self._head_side = self._new_stream(device, (self._side,))
        return self._head_side

    def _split_buffers(self, pointcloud):
        """Persistent state of the split sa1 level (one set per batch shape): head (temp, idx) and tail (temp, idx)."""
        B, n = pointcloud.shape[0], pointcloud.shape[1]
        key = ("split", B, n, str(pointcloud.device))
        bufs = self.__dict__.setdefault("_plan_bufs", {})
        if key not in bufs:
            mk = lambda shape, dt: torch.zeros(shape, device=pointcloud.device, dtype=dt)
            bufs[key] = {"head_temp": mk((B, n), torch.float32), "head_idx": mk((B, self.sa1.npoint), torch.int32),
                         "tail_temp": mk((B, n), torch.float32), "tail_idx": mk((B, self.sa1.npoint), torch.int32)}
        return bufs[key]

    def prefetch_head(self, pointcloud, rounds, trusted=False, footprint="small"):
        """Rounds [0, rounds) of the sa1 sampling of a batch TWO steps ahead, on a second side stream, into the persistent
        head state.  hand_over_head() -- or the next prefetch(..., resume=True), which calls it when no state has been handed
        over -- makes it the state a resumed chain continues.  trusted: as prefetch().  footprint: "small" (default) / "fast":
        a head runs next to a tail and, with a teacher, next to two more samplings, and every multi-workgroup sampling
        launch needs all workgroups of its scenes resident at once: the small footprint keeps four of them at 8 scenes
        on 4 x 8 x 3 = 96 compute units instead of 160."""
        if not pointcloud.is_cuda:
            return
        ext = pointnet2_utils._ext
        if not hasattr(ext, "furthest_point_sampling_resume"):
            raise RuntimeError("prefetch_head: this binding cannot resume a sampling")
        npoint = self.sa1.npoint
        rounds = int(rounds)
        if not 1 <= rounds <= npoint:
            raise ValueError(f"prefetch_head: rounds must be in [1, {npoint}]")
        main = torch.cuda.current_stream(pointcloud.device)
        side = self._head_stream(pointcloud.device)
        side.wait_stream(main)
        st = self._split_buffers(pointcloud)
        if not torch.cuda.is_current_stream_capturing():
            pointcloud.record_stream(side)
            for t in (st["head_temp"], st["head_idx"]):
                t.record_stream(side)
        with torch.cuda.stream(side), torch.no_grad():
            xyz = pointcloud[..., 0:3].contiguous()
            st["head_temp"].fill_(1e10)
            ext.furthest_point_sampling_resume(xyz, st["head_idx"], st["head_temp"], 0, rounds, small_footprint=footprint == "small")
            ev = torch.cuda.Event()
            ev.record(side)
        self._head = Head(rounds, ev, self._key(pointcloud), trusted, pointcloud)

    def hand_over_head(self):
        """Head state -> tail state on the current stream (temp and idx[:, :rounds]: 1.3 MB at 8 x 40 000 points), ordered
        behind the head.  The head buffers are free for the next head afterwards."""
        head, self._head = self._head, None
        if head is None:
            raise RuntimeError("hand_over_head: no head was sampled (prefetch_head)")
        st = self._split_buffers(head.src)
        cur = torch.cuda.current_stream(head.src.device)
        cur.wait_event(head.event)
        k = head.rounds
        with torch.no_grad():
            st["tail_temp"].copy_(st["head_temp"])
            st["tail_idx"][:, :k].copy_(st["head_idx"][:, :k])
        self._tail = Tail(k, head.key, head.trusted)

    def _take_tail(self, pointcloud, trusted):
        """The handed-over tail state if it is this cloud's (or vouched for), else None: the level is sampled from 0."""
        tail, self._tail = self._tail, None
        if tail is not None and not (tail.trusted or trusted or tail.key == self._key(pointcloud)):
            tail = None                    # the head of some other cloud
        if tail is not None:
            self.resumed_levels += 1
        return tail

    @staticmethod
    def _key(xyz_src):
        return (xyz_src.data_ptr(), xyz_src._version, tuple(xyz_src.shape))

    def _plan_buffers(self, pointcloud):
        """Persistent index buffers of the plan (one set per batch shape), so that a plan started inside a
        captured hipGraph lands at the same addresses on every replay."""
        key = (pointcloud.shape[0], str(pointcloud.device))
        bufs = self.__dict__.setdefault("_plan_bufs", {})
        if key not in bufs:
            bufs[key] = [torch.zeros((pointcloud.shape[0], getattr(self, n).npoint), device=pointcloud.device,
                                     dtype=torch.int32) for n in _SA_NAMES]
        return bufs[key]

    # Grouping ahead of the stages (round 5).  The centres, the ball-query indices and the row plan of a stage depend on
    # coordinates only, like the sampling itself: a chain started by prefetch() appends them for all four stages (gather_xyz,
    # ball query, the plan's three small kernels: ~0.25 ms and ~14 launches that otherwise sit on the main stream between the
    # stages' GEMMs) and leaves them in ONE flat persistent buffer (chain_plan.chain_layout says where); forward() takes it
    # with one copy and hands every stage its chain_plan.StageAhead on the index tensor (`inds.omnipq_stage_ahead`).  Same
    # kernels, same inputs: identical results.  Switch: GROUP_AHEAD.

    def _chain_layout(self, B, n_points):
        """Where the pieces of a chain launched NOW lie: sa_fused's switches are read here, at launch time."""
        import sa_fused
        stages = tuple((n, getattr(self, n).npoint, getattr(self, n).nsample) for n in _SA_NAMES)
        planned = tuple(sa_fused.plan_static_ok(S, B * M * S) for _, M, S in stages)
        words = tuple(sum(sa_fused.plan_words(B, M, B * M * S)) for _, M, S in stages)
        extra = next(iter(self.plan_extra.items())) if self.plan_extra else None
        return chain_plan.chain_layout(B, n_points, stages, planned, words, _FP_PAIRS, extra, sa_fused.PLAN_GROUP)

    def _ahead_buffer(self, pointcloud):
        """-> (the persistent flat buffer of this batch shape, the layout of a chain launched now)"""
        B, n = pointcloud.shape[0], pointcloud.shape[1]
        key = ("group", B, n, str(pointcloud.device))
        store = self.__dict__.setdefault("_plan_bufs", {})
        layout = self._chain_layout(B, n)
        if key not in store or store[key].numel() < layout.total:
            store[key] = torch.zeros((layout.total,), device=pointcloud.device, dtype=torch.int32)
        return store[key], layout

    def _launch_plan(self, pointcloud, trusted=False, small=False, group=False, resume=False):
        """FPS chain for `pointcloud` on the side stream -> ChainPlan; the caller's stream has to wait on events[i] before
        using inds[i].
        group: also the stages' centres / ball queries / row plans (GROUP_AHEAD) -> ChainPlan.ahead.
        resume: the sa1 level continues the handed-over tail state (see prefetch_head) instead of sampling from 0."""
        tail = self._take_tail(pointcloud, trusted) if resume else None
        main = torch.cuda.current_stream(pointcloud.device)
        side = self._side_stream(pointcloud.device)
        side.wait_stream(main)
        bufs = self._plan_buffers(pointcloud)
        key = self._key(pointcloud)
        ext = pointnet2_utils._ext
        product = hasattr(ext, "set_timing_sink")          # the product binding (writes in place), not a stand-in
        flat, layout, views = None, None, None
        if group and GROUP_AHEAD and product:
            flat, layout = self._ahead_buffer(pointcloud)
            views = chain_plan.chain_views(flat, layout, pointcloud.shape[0])
        if not torch.cuda.is_current_stream_capturing():
            # The cloud and the persistent index buffers come from the caller's stream's pool but are read / written
            # by the sampling stream: if either dies while a plan is still running (a model dropped right after a
            # prefetch -- seen in the test-suite as FPS indices landing in the next test's fresh tensor), the
            # allocator must not hand the block out before the sampling stream is done with it.
            held = [pointcloud] + bufs + ([flat] if flat is not None else [])
            if tail is not None:
                held += list(self._split_buffers(pointcloud).values())
            for t in held:
                t.record_stream(side)
        with torch.cuda.stream(side), torch.no_grad():
            inds, events, extra, srcs = self._sample_levels(ext, product, pointcloud, bufs, tail, small, views, side)
            ahead = None
            if views is not None:
                # behind every sampling level (their events fire first): ball query and row plan per stage
                ahead = self._group_levels(ext, flat, layout, views, inds, srcs, extra, side)
        return ChainPlan(key, pointcloud, trusted, inds, events, extra, ahead)

    def _sample_levels(self, ext, product, pointcloud, bufs, tail, small, views, side):
        """The four sampling levels (and the extra one) on the current = side stream, an event behind each.  views: of the
        chain's flat buffer; the levels' centres go there and the coordinates each level sampled from are kept for the
        grouping.  -> (inds per level, events per level, ExtraLevel | None, source coordinates per level)"""
        inds_all, events, srcs, extra = [], [], [], None
        xyz = pointcloud[..., 0:3].contiguous()
        for li, name in enumerate(_SA_NAMES):
            npoint = getattr(self, name).npoint
            if li == 0 and tail is not None:
                # the level's rounds [k, npoint) from the tail state; the picks [0, k) move into the plan's buffer
                st, k = self._split_buffers(pointcloud), tail.rounds
                inds = bufs[0]
                inds[:, :k].copy_(st["tail_idx"][:, :k])
                ext.furthest_point_sampling_resume(xyz, inds, st["tail_temp"], k, npoint - k, small_footprint=small)
            elif product:
                inds = ext.furthest_point_sampling(xyz, npoint, out=bufs[li], small_footprint=small)
            else:
                inds = ext.furthest_point_sampling(xyz, npoint)
            ev = torch.cuda.Event()
            ev.record(side)
            inds_all.append(inds)
            events.append(ev)
            if views is not None:
                src = xyz.contiguous()
                xyz = ext.gather_xyz(src, inds, out=views.stages[li].centres)
                srcs.append(src)
            elif name != "sa4":
                if hasattr(ext, "gather_xyz"):
                    xyz = ext.gather_xyz(xyz.contiguous(), inds)
                else:
                    xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), inds) \
                        .transpose(1, 2).contiguous()
            if self.plan_extra and name in self.plan_extra:
                n_extra = self.plan_extra[name]
                buf = self.__dict__.setdefault("_plan_bufs", {}).setdefault(
                    ("extra", name, pointcloud.shape[0], str(pointcloud.device)),
                    torch.zeros((pointcloud.shape[0], n_extra), device=pointcloud.device, dtype=torch.int32))
                if not torch.cuda.is_current_stream_capturing():
                    buf.record_stream(side)
                e_inds = ext.furthest_point_sampling(xyz, n_extra, out=buf) if product else \
                    ext.furthest_point_sampling(xyz, n_extra)
                e_ev = torch.cuda.Event()
                e_ev.record(side)
                extra = ExtraLevel(name, e_inds, e_ev)
        return inds_all, events, extra, srcs

    def _group_levels(self, ext, flat, layout, views, inds, srcs, extra, side):
        """Behind the sampling levels, on the current = side stream: every stage's ball query, row plan and backward CSR,
        the FP modules' 3-NN weights and CSR, and the sampled indices themselves, all into the views of `flat` -> Ahead"""
        import sa_fused
        planned = []
        for name, st, src, picked in zip(_SA_NAMES, views.stages, srcs, inds):
            mod = getattr(self, name)
            st.inds.copy_(picked)
            with sa_fused._tagged("@sa", name):
                ext.ball_query(st.centres, src, mod.radius, mod.nsample, out=st.idx)
                rp = sa_fused.make_row_plan(st.idx, st.idx.numel(), into=st.plan_state) if st.plan_state is not None else None
                if st.csr is not None:
                    # in the row space the stage will run in: compact under a plan (a planned stage = training)
                    sa_fused.build_csr_ahead(st.idx, src.shape[1], rp if mod.training else None, st.csr.offsets, st.csr.order)
            planned.append(rp is not None and mod.training)
        for fp in views.fps:
            ext.three_nn_weights(fp.unknown, fp.known, out=(fp.weight, fp.idx))
            sa_fused.build_csr_ahead(fp.idx, fp.known.shape[1], None, fp.csr.offsets, fp.csr.order)
        if views.extra is not None and extra is not None and extra.name == layout.extra.name:
            views.extra.copy_(extra.inds)
        event = torch.cuda.Event()
        event.record(side)
        return Ahead(flat, event, layout, tuple(planned))

    def prefetch(self, pointcloud, trusted=False, at_next_forward=False, footprint=None, resume=False):
        """Start the sampling plan of a FUTURE batch now (e.g. while the current batch is in backward).
        A later forward() on the very same tensor picks the result up; any other input recomputes.
        trusted=True: the next forward() takes the plan whatever tensor it is given (the caller vouches
        that the contents match -- used when a captured graph feeds forward() from a static buffer).
        at_next_forward=True: do not start now but inside the NEXT forward(), right after it has taken (and copied) the plan
        it runs on -- the earliest point at which the plan's persistent index buffers may be overwritten.  The sampling
        chain (7 ms of dependent argmax rounds for 8 x 40 000 points) then has the whole step to hide under, forward
        included, instead of the backward pass only.
        footprint: "small" runs the 40 000-point level on 3 instead of 5 compute units per scene with ~40 % longer rounds
        (_ext.furthest_point_sampling(small_footprint=True): same indices) -- right when the chain ends well before the
        step it hides under, which is the default for at_next_forward; "fast" otherwise (e.g. two chains per step).
        resume=True: the sa1 level continues at the round where prefetch_head() of this cloud stopped (the state handed over
        by hand_over_head(); handed over here if that has not happened yet).  Without a head, or with the head of another
        cloud, the level is sampled from 0 as usual (`resumed_levels` counts the levels that did continue one)."""
        if not pointcloud.is_cuda:
            return
        small = (footprint or ("small" if at_next_forward else "fast")) == "small"
        if resume and self._tail is None and self._head is not None:
            self.hand_over_head()
        if at_next_forward:
            self._pending = Pending(pointcloud, trusted, small, True, resume)
        else:
            self._plan = self._launch_plan(pointcloud, trusted, small, True, resume)

    def forget_plan(self):
        """Drop the HOST-side record of a plan in flight / pending (not the device work).  A captured step replays its
        sampling chains from the graph; the plan record its capture run (or an up-front `prefetch` before a replay) left behind
        is marked `trusted` and would hand a LATER eager forward() -- an evaluation pass between two training steps -- the
        indices of whatever batch the static buffers held last.  train_step.CapturedStep calls this after the capture and
        after every replay."""
        self._plan = None
        self._pending = None
        self._extra = None
        self._head = None
        self._tail = None

    def join(self, device=None):
        """Make the current stream wait for everything queued on the sampling streams."""
        for side in (self._side, self._head_side):
            if side is not None:
                torch.cuda.current_stream(side.device).wait_stream(side)

    def take_extra(self, name):
        """Indices of the plan's extra level `name` for the batch just run through forward(), or None."""
        extra, self._extra = self._extra, None
        if extra is None or extra.name != name:
            return None
        if extra.event is None:
            return extra.inds               # forward() copied it out of the plan's buffer already
        torch.cuda.current_stream(extra.inds.device).wait_event(extra.event)
        return extra.inds.clone()           # the plan's buffer is reused by the next plan

    def _take_plan(self, pointcloud):
        if not pointcloud.is_cuda or os.environ.get("OMNIPQ_SAMPLING_PLAN", "1") == "0":
            return None
        plan = self._plan
        self._plan = None
        if plan is None or not (plan.trusted or plan.key == self._key(pointcloud)):
            plan = self._launch_plan(pointcloud)
        return plan

    def _take_ahead(self, plan, pointcloud):
        """What the chain made ahead of the stages (GROUP_AHEAD): one copy of its flat buffer, read with the layout it was
        filled with.  -> (indices per stage, StageAhead per stage, the plan without what travelled in that copy)"""
        import sa_fused
        flat, event, layout, planned = plan.ahead
        torch.cuda.current_stream(pointcloud.device).wait_event(event)
        views = chain_plan.chain_views(flat.clone(), layout, pointcloud.shape[0], planned)
        stages = list(views.stages)
        if layout.plan_group != sa_fused.PLAN_GROUP:       # plans (and the CSRs in their row space) of another group size: not these
            stages = [s._replace(plan_state=None, csr=None, planned=False) for s in stages]
        if views.extra is not None and plan.extra is not None and plan.extra.name == layout.extra.name:
            self._extra = ExtraLevel(layout.extra.name, views.extra, None)
            plan = plan._replace(extra=None)
        # A record rides on one of its own tensors (the FP modules find theirs on the unknown centres, the stages on the
        # indices): it goes without that field, or tensor and record would keep each other -- and the whole copy -- alive
        # until a garbage collection.
        for fp in views.fps:
            fp.unknown.omnipq_fp_ahead = fp._replace(unknown=None)
        # the indices travel in the same copy: nothing else of this plan is read
        return [s.inds for s in stages], [s._replace(inds=None) for s in stages], plan._replace(inds=None)

    def _taken(self, pointcloud):
        """The sampling plan of this batch, taken in forward()'s order: yields (indices | None, StageAhead | None) per stage.
        Before the first stage: the chain's flat buffer in one copy (_take_ahead); with a chain pending, everything else the
        plan still holds is copied and the pending chain launched (it reuses the plan's buffers).  Otherwise the indices of
        a stage are waited for and copied when that stage is asked for, so a later level keeps sampling under the stages in
        front of it.  The extra level lands in self._extra (take_extra)."""
        plan = self._take_plan(pointcloud)
        self._extra = plan.extra if plan is not None else None
        inds, aheads = [None] * 4, [None] * 4
        if plan is not None and plan.ahead is not None:
            inds, aheads, plan = self._take_ahead(plan, pointcloud)
        pending, self._pending = self._pending, None
        if pending is not None:
            if plan is not None:
                # the next plan starts below and reuses this plan's buffers: copy everything it holds NOW
                cur = torch.cuda.current_stream(pointcloud.device)
                if plan.inds is not None:                  # (else they came with the chain's flat buffer)
                    for li in range(4):
                        cur.wait_event(plan.events[li])
                        inds[li] = plan.inds[li].clone()
                if plan.extra is not None:
                    cur.wait_event(plan.extra.event)
                    self._extra = ExtraLevel(plan.extra.name, plan.extra.inds.clone(), None)
                plan = None
            self._plan = self._launch_plan(*pending)
        for li in range(4):
            if plan is not None and plan.inds is not None:
                torch.cuda.current_stream(pointcloud.device).wait_event(plan.events[li])
                inds[li] = plan.inds[li].clone()           # the plan's buffers are reused by the next plan
            yield inds[li], aheads[li]

    def _break_up_pc(self, pc):
        xyz = pc[..., 0:3].contiguous()
        features = pc[..., 3:].transpose(1, 2).contiguous() if pc.size(-1) > 3 else None
        return xyz, features

    def forward(self, pointcloud, end_points=None):
        if not end_points:
            end_points = {}
        xyz, features = self._break_up_pc(pointcloud)
        for name, (inds, ahead) in zip(_SA_NAMES, self._taken(pointcloud)):
            if ahead is not None and inds is not None:
                inds.omnipq_stage_ahead = ahead
            xyz, features, inds = getattr(self, name)(xyz, features, inds)
            if name in ("sa1", "sa2"):          # the reference records inds for these two only
                end_points[name + "_inds"] = inds
            end_points[name + "_xyz"] = xyz
            end_points[name + "_features"] = features

        features = self.fp1(end_points["sa3_xyz"], end_points["sa4_xyz"],
                            end_points["sa3_features"], end_points["sa4_features"])
        features = self.fp2(end_points["sa2_xyz"], end_points["sa3_xyz"],
                            end_points["sa2_features"], features)
        end_points["fp2_features"] = features
        end_points["fp2_xyz"] = end_points["sa2_xyz"]
        num_seed = end_points["fp2_xyz"].shape[1]
        # seeds are the first num_seed FPS picks of sa1, i.e. indices into the input cloud
        end_points["fp2_inds"] = end_points["sa1_inds"][:, 0:num_seed]
        end_points["seed_inds"] = end_points["fp2_inds"]
        end_points["seed_xyz"] = end_points["fp2_xyz"]
        end_points["seed_features"] = end_points["fp2_features"]
        return end_points
