"""The fast training step as a product API: one object that runs `model(inputs)` -> `criterion` -> `backward` of
`PQ_Transformer` the way the benchmark does -- captured once into a hipGraph and replayed, the ~130 weight gradients as a
few grouped launches (`sa_fused.deferred_wgrads`), the NEXT batch's furthest-point sampling chain started inside the
current forward on a side stream, and under `torch.distributed` the gradients reduced in two buckets of which the first
travels underneath the backbone's backward pass (`data_parallel.GradientBuckets`).

Where it goes in the reference's driver (train.py:456-576): the three lines

    end_points = model(inputs)                              # train.py:489
    loss, end_points = criterion(end_points, ...)           # train.py:497-503
    loss.backward()                                         # train.py:559

become `loss = stepper.step(batch, labels, next_inputs=next_batch)`; `optimizer.step()` (train.py:560-563) stays where
it is and finds the gradients in `.grad` of the bare model's parameters, averaged over the ranks.  INTEGRATION.md shows
the whole change.  The model is NOT wrapped in DistributedDataParallel: DDP reduces from per-parameter autograd hooks,
which a captured step with deferred weight gradients never fires (`deferred_wgrads` refuses DDP parameters).  With `CapturedStep(..., optimizer=optim.FusedAdamW(...))` the clip and the AdamW step of train.py:562-563 run inside
the captured step as well (three launches at its end, hyper-parameters in device memory) and only `scheduler.step()` stays --
unless the optimizer carries `lr_schedule=optim.LRSchedule(...)`, which its finalise launch steps on the device; with
`stats=` the reference's per-step `.item()` loop (train.py:580-586) becomes one more launch and one read per print_freq steps.

Launched kernel by kernel (`graph=False`, or under DDP) the same step is host-bound (about 2.3x slower at batch 8 x
40 000 points on MI355X); the capture is what makes the 650 dependent launches of 3-150 us run back to back.
"""
import gc

import torch
import torch.distributed as dist


def lookahead(iterable):
    """(item, next item or None) pairs: the captured step wants to know the batch AFTER the one it runs."""
    it = iter(iterable)
    try:
        cur = next(it)
    except StopIteration:
        return
    for nxt in it:
        yield cur, nxt
        cur = nxt
    yield cur, None


def _cloud(inputs):
    return inputs["point_clouds"] if isinstance(inputs, dict) else inputs


class CapturedStep:
    """stepper = CapturedStep(net, criterion, example_inputs, example_labels)
       loss = stepper.step(inputs, labels, next_inputs=...)         # gradients in net's parameters' .grad

    net              the bare PQ_Transformer (train mode).  `model` (default: net) is what is called -- pass a wrapper only if
                     it forwards to `net` without hooks of its own.
    criterion        criterion(end_points, labels) -> scalar loss tensor; must not read the device from the host
                     (loss_helper_pq.get_loss qualifies; `labels` is a dict of tensors or None).
    example_inputs   {'point_clouds': (B, N, 3 + C) f32 on the GPU} (or the tensor): fixes the batch shape; its contents
                     are only used for the warm-up steps.
    amp_dtype        torch.bfloat16 / torch.float16 / None (strict f32); loss_scale: static scale applied to the loss before
                     backward (fp16: 2^14, what torch.amp.GradScaler would settle on; gradients come back scaled), or
                     "dynamic": torch.amp.GradScaler's behaviour inside the step.  Accepted with
                     optimizer=optim.FusedAdamW(..., loss_scaler=optim.LossScaler(...)) and with nothing else (such an
                     optimizer in turn takes no numeric loss_scale other than 1).  The loss is multiplied by
                     optimizer.loss_scale, a device word (one multiply, as with a static scale: the step's launch count does
                     not change); the optimizer's finalise launch un-scales, skips a step whose norm is not finite, backs the
                     scale off then and grows it after growth_interval good steps, so a replay follows the scale the one
                     before it left.  Composes with step_freq=k (the scale is constant over an accumulation window),
                     teacher= / ema_in_step=True and buckets=.  Under data parallelism the gradients are all-reduced before
                     the optimizer's launches, so every rank forms the same norm from the same bits and takes the same
                     decision: the scales stay equal without a collective of their own (they start equal: same init_scale
                     or the same loaded scaler_state_dict()).  optimizer.scale_value / .growth_tracker read it back;
                     building the stepper leaves both where they were.
    graph            True: capture + replay; False: the same step launched eagerly (debugging, A/B).
    prefetch         "forward": the next batch's sampling chain starts inside forward() (default), "backward": between
                     forward and backward, None: no prefetch (every forward samples its own batch: +5 ms at 40 000 points).
    teacher          optional mean-teacher copy (train.py:480-491): its train-mode no-grad forward runs right after the
                     student's forward, BEFORE the criterion; with `teacher_to_criterion=True` the criterion is called as
                     criterion(end_points, labels, teacher_end_points) (train.py:530-538: the consistency loss reads both).
                     The weight averaging is NOT part of the captured step: call `stepper.update_teacher(global_step)`
                     after `optimizer.step()`, where the reference calls update_ema_variables (train.py:560-576) -- one
                     launch, alpha = min(1 - 1/(global_step + 1), ema) evaluated per call.  `ema` = the decay (a
                     (decay, step) pair is accepted for old callers; its step is ignored).
    ema_in_step      False (default): as above.  True (needs `teacher`, a scalar `ema` and optimizer=optim.FusedAdamW): the
                     averaging runs INSIDE the step, in the optimizer's finalise and update launches
                     (optimizer.attach_teacher(net, teacher, ema) is called here): alpha is formed on the device from a step
                     count that lives there, so every replay averages with its own alpha, on applying steps only.  The order
                     is the reference's -- the teacher's forward runs on the old weights, the averaging follows the update.
                     update_teacher() then raises; the first averaging uses global_step 1 (optimizer.set_global_step(i)
                     for a resumed run).  Building the stepper changes neither the teacher nor the global step.
    world / buckets  data parallelism: `buckets` = data_parallel.GradientBuckets(net, world, group) or None (single rank).
    defer            False: leave the weight gradients to autograd (needed under DistributedDataParallel).
    lookahead        1 (default): the sampling chain of the NEXT batch runs underneath this step, so one step contains a whole
                     chain.  2: the chain is spread over two steps -- this step runs the rounds [head_rounds, npoint) of the
                     next batch's sa1 level plus levels 2-4 on the sampling stream (the TAIL) and, side by side on a second
                     stream, the rounds [0, head_rounds) of the sa1 level of the batch AFTER the next (the HEAD, announced
                     as step(..., after_next_inputs=...)); after both have joined, the head state (running distances and picks:
                     1.3 MB at 8 x 40 000 points) is copied to where the next step's tail continues it.  A batch that was
                     not announced two calls ahead gets its head sampled in front of the replay.  Same indices either way.
                     Samplings in flight at once: 2 (4 with a teacher); each multi-workgroup launch needs every workgroup
                     of its scenes resident, so all pieces of the split step use the small footprint (3 compute units per
                     40 000-point scene: 4 x 8 x 3 = 96 of 256 at batch 8, against 160 with the fast one) unless `fps_footprint`
                     says otherwise.  Needs prefetch="forward".
    head_rounds      lookahead=2: where the sa1 level is cut.  None = 0.50 x its npoint (1024 of 2048), the best MEASURED cut on
                     the mean-teacher step (profiles/fps_resume_ab.txt: 12.35 ms against 13.15 at 0.70 x -- the value derived
                     from the chain's proportions, (6.2 / 2) / 4.44 -- and 13.86 at 0.85 x; the plain step preferred 0.70 x by
                     0.06 ms).  Neither beat lookahead=1 on this runtime (10.97 ms; plain step 7.77 vs 7.81): opt-in.
    optimizer        None (default): the step ends with the gradients in `.grad`, the caller clips and steps.  An
                     optim.FusedAdamW over net's parameters: gradient clipping + AdamW (train.py:562-563) become the last
                     three launches of the step body, on the main stream behind the deferred weight-gradient flush and the
                     bucket all-reduce (no fork, no join of their own), captured with it.  Its hyper-parameters live in
                     device memory: step() stages what an LR scheduler wrote into `param_groups`
                     (optimizer.sync_hyperparameters()) in front of the replay, so scheduler.step() stays where it is and
                     update_teacher() is still called after step().  loss_scale != 1 sets optimizer.grad_scale =
                     1 / loss_scale; a step whose gradient norm is not finite leaves the weights alone (optimizer.skipped).
                     Building the stepper changes neither parameters nor optimiser state.  `stepper.grad_total_norm` is
                     the device tensor clip_grad_norm_ would have returned.
    step_freq        gradient accumulation (the reference's step_freq, train.py:493-494 and :562-576): k > 1 is accepted with
                     optimizer=optim.FusedAdamW(..., accum_steps=k) and with nothing else -- every step still starts from
                     empty gradients, the SUM lives in the optimizer's accumulator.  Every step() is then one micro-batch and
                     one replay of the same graph: the micro-batch counter is a device word the captured launches read.
                     `stepper.is_update_step` (a host bool, valid once step() has returned) says whether that call
                     applied the sum: call scheduler.step() and update_teacher() only then (an optimizer built with
                     lr_schedule=optim.LRSchedule(...) steps its schedule on the device, on those calls by itself).  The
                     gradients are summed, as in the reference (grad_scale = 1 / k for the mean).  With `buckets` every
                     micro-batch's gradients are
                     all-reduced before they are accumulated: the same sum, k times the communication (an all-reduce
                     deferred to the k-th micro-batch is not implemented).  A host-stepped optimizer accumulates outside:
                     step_freq stays 1, the caller adds `.grad` up after each step().
    stats            None, or a callable returning the mapping of device scalars the step reports once the criterion has run
                     (`lambda: objective.stats`, or a selection of stepper.end_points): the reference's stat_dict loop
                     (train.py:578-586) as ONE launch at the end of the step body, behind the optimizer's (it reads their
                     apply mark and the norm), captured with it.  `stepper.stats` is the step_stats.StepStats: keys are
                     chosen by train.py:581's rule, `grad_norm` joins with an in-graph optimizer, only applying steps are
                     accumulated, and `stepper.stats.read()` every print_freq steps is the loop's one host read.  The launch
                     is on the main stream: lookahead=2 and buckets= need nothing special.  graph=False runs it eagerly.
    """

    def __init__(self, net, criterion, example_inputs, example_labels=None, *, model=None, amp_dtype=torch.bfloat16,
                 loss_scale=1.0, graph=True, prefetch="forward", fps_footprint=None, teacher=None, teacher_example=None,
                 ema=None, buckets=None, defer=True, warmup=3, distributed=False, before_capture=None,
                 teacher_to_criterion=False, lookahead=1, head_rounds=None, optimizer=None, step_freq=1, ema_in_step=False,
                 stats=None):
        if optimizer is not None:
            import optim
            if not isinstance(optimizer, optim.FusedAdamW):
                raise TypeError("CapturedStep(optimizer=...): an optim.FusedAdamW or None -- any other optimizer steps from the "
                                "host, after step()")
        accum_steps = optimizer.accum_steps if optimizer is not None else 1
        if isinstance(step_freq, bool) or not isinstance(step_freq, int) or step_freq < 1 or step_freq != accum_steps:
            raise ValueError(f"CapturedStep: step_freq={step_freq!r} with " +
                             (f"an optimizer built with accum_steps={accum_steps}" if optimizer is not None
                              else "no in-graph optimizer") +
                             " -- every step starts from empty gradients, so gradient accumulation over k micro-batches "
                             "needs optimizer=optim.FusedAdamW(accum_steps=k) together with step_freq=k (a host-stepped "
                             "optimizer accumulates `.grad` itself after each step(), with step_freq=1)")
        self.step_freq = step_freq
        self.is_update_step = False
        scaler = optimizer.loss_scaler if optimizer is not None else None
        self.dynamic_scale = isinstance(loss_scale, str)
        if (self.dynamic_scale and (loss_scale != "dynamic" or scaler is None)) or \
                (not self.dynamic_scale and scaler is not None and float(loss_scale) != 1.0):
            raise ValueError(f"CapturedStep: loss_scale={loss_scale!r} with " +
                             ("an optimizer built with " + ("a loss_scaler" if scaler is not None else "no loss_scaler")
                              if optimizer is not None else "no in-graph optimizer") +
                             " -- a scale that backs off and grows lives in the optimizer's device memory, so "
                             'loss_scale="dynamic" needs optimizer=optim.FusedAdamW(loss_scaler=optim.LossScaler(...)), and '
                             "such an optimizer takes no second, static scale (a number other than 1) on top of its own")
        if self.dynamic_scale:
            loss_scale = 1.0             # the loss is multiplied by optimizer.loss_scale, a device tensor (_backward)
        if optimizer is not None:
            if float(loss_scale) != 1.0:
                optimizer.grad_scale = 1.0 / float(loss_scale)
        self.optimizer = optimizer
        self.grad_total_norm = optimizer.grad_total_norm if optimizer is not None else None
        if stats is not None and not callable(stats):
            raise TypeError("CapturedStep(stats=...): a callable returning the mapping of the step's device scalars (for "
                            "instance `lambda: objective.stats`) or None")
        self._stats_source = stats
        self.stats = None
        if stats is not None:
            import step_stats
            self.stats = step_stats.StepStats()
        if lookahead not in (1, 2):
            raise ValueError("CapturedStep: lookahead is 1 or 2")
        if lookahead == 2 and prefetch != "forward":
            raise ValueError('CapturedStep: lookahead=2 needs prefetch="forward"')
        self.lookahead = lookahead
        self.head_rounds = None
        if lookahead == 2:
            npoint = net.backbone.sa1.npoint
            self.head_rounds = int(0.50 * npoint) if head_rounds is None else int(head_rounds)
            if not 1 <= self.head_rounds < npoint:
                raise ValueError(f"CapturedStep: head_rounds must be in [1, {npoint})")
            if fps_footprint is None:
                fps_footprint = "small"
        self.net, self.model, self.criterion = net, (model if model is not None else net), criterion
        self.amp_dtype, self.scale = amp_dtype, float(loss_scale)
        self.prefetch_at, self.footprint = prefetch, fps_footprint
        self.teacher = teacher
        if isinstance(ema, (tuple, list)):
            # (decay, step) was the contract while the averaging ran inside step(); the step value would be dropped silently
            # and -- if update_teacher() is never called -- the teacher would stay frozen
            raise TypeError("CapturedStep(ema=...): pass the decay alone and call update_teacher(global_step) after "
                            "optimizer.step(); the (decay, step) pair of earlier versions is no longer accepted")
        self.ema = ema
        self.ema_in_step = bool(ema_in_step)
        if self.ema_in_step:
            if teacher is None or optimizer is None or isinstance(ema, bool) or not isinstance(ema, (int, float)):
                raise ValueError("CapturedStep(ema_in_step=True): the teacher is averaged by the optimizer's own launches, so it "
                                 "needs teacher=, a scalar ema= decay and optimizer=optim.FusedAdamW(...)")
            # before the warm-up: its eager steps build the tables the captured launches read
            optimizer.attach_teacher(net, teacher, ema)
        self.teacher_to_criterion = bool(teacher_to_criterion)
        self.teacher_end_points = None
        self._grads = None             # graph mode: (parameter, static gradient tensor) pairs, re-attached after every replay
        self.buckets, self.defer = buckets, defer
        self.distributed = distributed
        pc = _cloud(example_inputs)
        self.cur, self.nxt = pc.clone(), pc.clone()
        self.lab = {k: v.clone() for k, v in example_labels.items()} if example_labels is not None else None
        self.nxt2 = pc.clone() if lookahead == 2 else None
        self.cur_t = self.nxt_t = self.nxt2_t = None
        if teacher is not None:
            tpc = _cloud(teacher_example if teacher_example is not None else example_inputs)
            self.cur_t, self.nxt_t = tpc.clone(), tpc.clone()
            self.nxt2_t = tpc.clone() if lookahead == 2 else None
        self.graph = None
        self.static_loss = None
        self.end_points = None
        self.launch = "eager"
        self.replays = 0
        self._promised = None          # the tensor announced as `next_inputs` by the previous call (kept alive: compared with `is`)
        self._have_next = False        # does `nxt` (and the plan in flight) hold the batch the next call will run?
        self._promised2 = None         # lookahead=2: the tensor announced as `after_next_inputs` by the previous call
        if graph:
            self._capture(warmup, before_capture)

    # ---- the step body (what is captured) ----------------------------------------------------------------------------------
    def _backward(self, loss):
        import sa_fused
        if self.buckets is not None:
            self.buckets.collectives = 0
        if self.dynamic_scale:
            loss = loss * self.optimizer.loss_scale      # the device word the optimizer's finalise launch maintains
        elif self.scale != 1.0:
            loss = loss * self.scale
        if self.defer:
            with sa_fused.deferred_wgrads(on_early_flush=self.buckets.on_early_flush if self.buckets is not None else None):
                loss.backward()
        else:
            loss.backward()
        if self.buckets is not None:
            self.buckets.finish()

    TEACHER_FIRST = True        # the teacher's forward in front of the student's (see _body)

    def _teacher_forward(self, batch):
        import dropout_state
        with torch.no_grad(), torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype is not None), \
                dropout_state.STATE.use("teacher"):
            return self.teacher({"point_clouds": batch})            # train mode, no grad (train.py:462, 490-491)

    def _body(self, cur, nxt, lab, cur_t, nxt_t, trusted, nxt2=None, nxt2_t=None):
        """forward + loss (+ teacher forward) + backward (+ EMA) on `cur`, with the sampling plan of `nxt` started on the
        side stream.  trusted: the plan in flight IS the plan of `cur` whatever tensor object forward() is handed.
        lookahead=2: the chain of `nxt` continues the head sampled a step ago, and the head of `nxt2` runs next to it."""
        net, teacher = self.net, self.teacher
        for p in net.parameters():
            p.grad = None
        early = self.prefetch_at == "forward" and nxt is not None
        split = self.lookahead == 2
        if early and not split:
            net.prefetch({"point_clouds": nxt}, trusted=trusted, at_next_forward=True, footprint=self.footprint)
            if teacher is not None:
                teacher.prefetch({"point_clouds": nxt_t}, trusted=trusted, at_next_forward=True, footprint=self.footprint)
        heads = []
        if split:
            if early:
                net.prefetch({"point_clouds": nxt}, trusted=trusted, at_next_forward=True, footprint=self.footprint, resume=True)
                if teacher is not None:
                    teacher.prefetch({"point_clouds": nxt_t}, trusted=trusted, at_next_forward=True, footprint=self.footprint,
                                     resume=True)
            if nxt2 is not None:
                # the heads fork from (and join to) THIS stream, not from inside the sampling streams
                net.prefetch_head({"point_clouds": nxt2}, self.head_rounds, trusted=trusted, footprint=self.footprint)
                heads.append(net)
                if teacher is not None:
                    teacher.prefetch_head({"point_clouds": nxt2_t}, self.head_rounds, trusted=trusted, footprint=self.footprint)
                    heads.append(teacher)
        tep = None
        if teacher is not None and self.TEACHER_FIRST:
            # The two forwards are independent (train.py:489-491 runs the student's first; nothing reads one from the other
            # before the losses).  The teacher's goes FIRST here: its next sampling chain starts inside its forward, and behind
            # the student's forward it started ~2.7 ms into the step and ended after everything else -- the chain, not the
            # main stream, set the step's length (11.5 ms).  In front, both chains have the whole step to hide under.
            tep = self._teacher_forward(cur_t)
        with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype is not None):
            ep = self.model({"point_clouds": cur})
        if teacher is not None:
            if tep is None:
                tep = self._teacher_forward(cur_t)              # train.py:489-491: before the losses, which may read both
            self.teacher_end_points = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in tep.items()} \
                if isinstance(tep, dict) else None
        with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype is not None):
            loss = self.criterion(ep, lab, self.teacher_end_points) if (teacher is not None and self.teacher_to_criterion) \
                else self.criterion(ep, lab)
        # the outputs, detached: in graph mode static tensors that every replay rewrites in place.  (Detached on purpose:
        # holding the attached tensors -- i.e. the step's autograd graph with its custom nodes -- past the end of a capture
        # made hipStreamEndCapture segfault; the nodes must die inside the capture, as they do when only the loss leaves.)
        self.end_points = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in ep.items()} if isinstance(ep, dict) else None
        if self.prefetch_at == "backward" and nxt is not None:
            net.prefetch({"point_clouds": nxt}, trusted=trusted)
            if teacher is not None:
                teacher.prefetch({"point_clouds": nxt_t}, trusted=trusted)
        self._backward(loss)
        if self.optimizer is not None:
            # clip + AdamW: three launches on this stream, behind the weight-gradient flush and the bucket all-reduce
            if not self._capturing:
                self.optimizer.sync_hyperparameters()
            self.optimizer.launch()
        if self.stats is not None:
            # behind the optimiser's launches on this stream: it reads their apply mark and the norm
            self.stats.accumulate(self._stats_source(), self.optimizer)
        if not self._capturing:
            for m in heads:
                m.hand_over_head()                   # (this stream waits for the head; the host does not)
            return loss                              # eager mode: the plan keeps running underneath whatever comes next
        net.join_prefetch()
        if teacher is not None:
            teacher.join_prefetch()
        for m in heads:
            m.hand_over_head()                       # head state -> the state the next step's chain continues
        return loss

    def update_teacher(self, global_step):
        """ema_model <- alpha * ema_model + (1 - alpha) * model, alpha = min(1 - 1/(global_step + 1), decay): the
        reference's update_ema_variables (train.py:435-439), to be called where the reference calls it -- after
        optimizer.step() (train.py:560-576).  One launch on the current stream, outside the captured step: alpha is a
        kernel ARGUMENT and changes with every call, which a replayed launch could not follow."""
        if self.ema_in_step:
            raise RuntimeError("CapturedStep.update_teacher: this stepper was built with ema_in_step=True -- every applying step "
                               "averages the teacher inside the optimizer's launches, a second averaging would count twice")
        if self.teacher is None or self.ema is None:
            return None
        self._steps_unaveraged = 0
        import ema as _ema
        return _ema.update_ema_variables(self.net, self.teacher, self.ema, global_step)

    _capturing = False

    def _capture(self, warmup, before_capture):
        import sa_fused
        net, teacher = self.net, self.teacher
        self._capturing = True
        # the warm-up steps run the model in train mode on the EXAMPLE batch: what they do to the BatchNorm running
        # statistics / step counters of both networks is undone after the capture
        keep = [(b, b.detach().clone()) for m in (net, teacher) if m is not None for b in m.buffers()]
        opt_saved = None
        if self.optimizer is not None:
            # ... and so is what the in-graph optimizer does to the parameters, its moments and its counters (ema_in_step: to
            # the teacher's parameters and the global step as well -- optimizer.snapshot() carries them)
            keep += [(p, p.detach().clone()) for g in self.optimizer.param_groups for p in g["params"]]
            opt_saved = self.optimizer.snapshot()
            self.optimizer.sync_hyperparameters()
        try:
            self.nxt.copy_(self.cur)
            if teacher is not None:
                self.nxt_t.copy_(self.cur_t)
            split = self.lookahead == 2
            if split:
                # the warm-up steps run the split body, so the exchange workspaces of BOTH sampling streams exist (they grow
                # on first use, which a capture cannot do) and the first of them finds a head to continue
                self.nxt2.copy_(self.cur)
                if teacher is not None:
                    self.nxt2_t.copy_(self.cur_t)
                self._sample_head_now()
            if self.prefetch_at is not None:
                net.prefetch({"point_clouds": self.nxt}, trusted=True)          # plan of the first batch
                if teacher is not None:
                    teacher.prefetch({"point_clouds": self.nxt_t}, trusted=True)
            for _ in range(max(int(warmup), 3)):          # eager warm-up: allocator pools, workspaces, weight arenas
                self.cur.copy_(self.nxt)
                if teacher is not None:
                    self.cur_t.copy_(self.nxt_t)
                self._body(self.cur, self.nxt if self.prefetch_at else None, self.lab, self.cur_t, self.nxt_t, True,
                           self.nxt2, self.nxt2_t)
            torch.cuda.synchronize()
            if self.distributed:
                _quiesce_process_groups(self.cur.device, (getattr(self.buckets, "group", None),))
            if before_capture is not None:
                before_capture()
            torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
            sa_fused.reset_pools()
            # A captured graph that died in a reference cycle (an earlier CapturedStep, say) must not be collected inside this
            # capture: on ROCm its destructor synchronises the device, which a capture in progress refuses, and an error
            # thrown from a destructor ends the process.  torch.cuda.graph itself no longer collects before it begins.
            gc.collect()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.static_loss = self._body(self.cur, self.nxt if self.prefetch_at else None, self.lab, self.cur_t,
                                              self.nxt_t, True, self.nxt2, self.nxt2_t)
            self.graph = graph
            self.launch = "hipGraph replay"
            self._have_next = True                   # `nxt` holds the example batch, its plan was started by the capture run
            # the gradients the graph writes: static tensors (views of the bucket buffers under data parallelism).  A
            # caller's optimizer.zero_grad() (set_to_none=True is torch's default) detaches them from the parameters, so
            # every replay hands them back.
            self._grads = [(p, p.grad) for p in net.parameters() if p.grad is not None]
            if self.optimizer is not None:
                self.optimizer.retarget()            # the table the captured launches read: the capture's own gradient tensors
                self.optimizer.restore(opt_saved)
            if self.stats is not None:
                self.stats.retarget()                # ... and the statistics' table at the capture's own scalars
                self.stats.reset()                   # the warm-up steps are in no window
            self._forget_plans()
            with torch.no_grad():
                for b, saved in keep:
                    b.copy_(saved)
        finally:
            self._capturing = False

    # ---- one training step -------------------------------------------------------------------------------------------------
    def _sample_head_now(self):
        """lookahead=2: head of the batch in `nxt`, sampled and handed over on the spot (no head of it is in flight)."""
        self.net.prefetch_head({"point_clouds": self.nxt}, self.head_rounds, trusted=True, footprint=self.footprint)
        self.net.hand_over_head()
        if self.teacher is not None:
            self.teacher.prefetch_head({"point_clouds": self.nxt_t}, self.head_rounds, trusted=True, footprint=self.footprint)
            self.teacher.hand_over_head()

    def step(self, inputs=None, labels=None, next_inputs=None, teacher_inputs=None, next_teacher_inputs=None,
             after_next_inputs=None, after_next_teacher_inputs=None):
        """Forward + loss + backward of `inputs`; returns the loss (graph mode: a static tensor, overwritten by the next
        call).  next_inputs: the batch the NEXT call will run (tensor / dict / callable(dst) filling the static buffer) -- its
        coordinate-only sampling runs underneath this step.  inputs=None or the very object announced as `next_inputs` last
        time: the announced batch is taken as is; any other input is copied in and its sampling plan recomputed up front
        (correct, and ~5 ms slower for that call at 40 000 points).  next_inputs=None: nothing to announce (last batch).
        after_next_inputs (lookahead=2 only): the batch of the call after the next; the head of its sampling runs underneath
        this step.  A `next_inputs` that was not announced this way one call earlier (the very object) has its head sampled
        in front of the replay."""
        if self.lookahead != 2 and (after_next_inputs is not None or after_next_teacher_inputs is not None):
            raise ValueError("CapturedStep.step: after_next_inputs needs a stepper built with lookahead=2")
        # will this call apply the (accumulated) gradients?  Known up front: the optimizer mirrors its device counter
        applies = self.optimizer is None or self.optimizer.micro == self.step_freq - 1
        if self.teacher is not None and self.ema is not None and applies and not self.ema_in_step:
            self._steps_unaveraged = getattr(self, "_steps_unaveraged", 0) + 1
            if self._steps_unaveraged == 4:
                import warnings
                warnings.warn("CapturedStep: a teacher and an EMA decay are set but update_teacher(global_step) has not been "
                              "called for three applying steps -- the teacher's weights are not being averaged (call it after "
                              "optimizer.step(), where the reference calls update_ema_variables)")
        self.is_update_step = applies
        if self.graph is None:
            return self._eager_step(inputs, labels, next_inputs, teacher_inputs, next_teacher_inputs, after_next_inputs,
                                    after_next_teacher_inputs)
        net, teacher = self.net, self.teacher
        pc = None if inputs is None else _cloud(inputs)
        announced = self._have_next and (pc is None or (self._promised is not None and self._promised[0] is pc
                                                        and self._promised[1] == pc._version))
        if announced:
            self.cur.copy_(self.nxt)
            if teacher is not None:
                self.cur_t.copy_(self.nxt_t)
        else:
            if pc is None:
                raise ValueError("CapturedStep.step: no batch was announced by the previous call; pass `inputs`")
            self.cur.copy_(pc)
            if teacher is not None:
                self.cur_t.copy_(_cloud(teacher_inputs if teacher_inputs is not None else inputs))
            if self.prefetch_at is not None:
                # the plan in flight belongs to some other batch: sample this one now, ahead of the replay
                net.prefetch({"point_clouds": self.cur}, trusted=True)
                net.join_prefetch()
                if teacher is not None:
                    teacher.prefetch({"point_clouds": self.cur_t}, trusted=True)
                    teacher.join_prefetch()
        if self.lab is not None:
            if labels is None:
                raise ValueError("CapturedStep.step: this step was captured with labels")
            for k, dst in self.lab.items():
                dst.copy_(labels[k])
        self._fill(self.nxt, next_inputs)
        if teacher is not None:
            self._fill(self.nxt_t, next_teacher_inputs if next_teacher_inputs is not None else next_inputs)
        if next_inputs is not None and not callable(next_inputs):
            t = _cloud(next_inputs)
            self._promised = (t, t._version)         # the object itself, kept alive until the next call: an address can be reused
        else:
            self._promised = None
        self._have_next = next_inputs is not None
        if self.lookahead == 2:
            t = None if (next_inputs is None or callable(next_inputs)) else _cloud(next_inputs)
            head_ahead = t is not None and self._promised2 is not None and self._promised2[0] is t \
                and self._promised2[1] == t._version
            if next_inputs is not None and not head_ahead:
                self._sample_head_now()              # the head in the tail state belongs to some other batch
            self._fill(self.nxt2, after_next_inputs)
            if teacher is not None:
                self._fill(self.nxt2_t, after_next_teacher_inputs if after_next_teacher_inputs is not None
                           else after_next_inputs)
            if after_next_inputs is not None and not callable(after_next_inputs):
                t2 = _cloud(after_next_inputs)
                self._promised2 = (t2, t2._version)
            else:
                self._promised2 = None
        if self.optimizer is not None:
            self.optimizer.sync_hyperparameters()    # what a scheduler wrote into param_groups since the last step
            self.optimizer._opt_called = True        # (torch's schedulers warn when they never see optimizer.step())
        self.graph.replay()
        self.replays += 1
        if self.optimizer is not None:
            self.optimizer.replayed()                # the host mirror of the micro-batch counter the replay advanced
        for p, g in self._grads:
            p.grad = g
        self._forget_plans()
        return self.static_loss

    def _forget_plans(self):
        """The replayed graph owns the sampling chains; what the capture run (or the up-front sampling of an unannounced batch)
        left in the networks' host-side plan records must not reach a later EAGER forward of the same network (an evaluation
        pass between steps would silently take the indices of another batch)."""
        for m in (self.net, self.teacher):
            if m is not None and hasattr(m, "forget_prefetch"):
                m.forget_prefetch()

    @staticmethod
    def _fill(dst, src):
        if src is None:
            return
        if callable(src):
            src(dst)
        else:
            dst.copy_(_cloud(src))

    def _eager_step(self, inputs, labels, next_inputs, teacher_inputs, next_teacher_inputs, after_next_inputs=None,
                    after_next_teacher_inputs=None):
        """The same sequence launched kernel by kernel (no static buffers: the caller's tensors are used directly)."""
        if inputs is None:
            raise ValueError("CapturedStep.step (eager): pass `inputs`")
        pc = _cloud(inputs)
        nxt = None
        if next_inputs is not None and not callable(next_inputs) and self.prefetch_at is not None:
            nxt = _cloud(next_inputs)
        t_cur = _cloud(teacher_inputs) if teacher_inputs is not None else pc
        t_nxt = _cloud(next_teacher_inputs) if next_teacher_inputs is not None else nxt
        nxt2 = t_nxt2 = None
        if self.lookahead == 2 and after_next_inputs is not None and not callable(after_next_inputs):
            nxt2 = _cloud(after_next_inputs)
            t_nxt2 = _cloud(after_next_teacher_inputs) if after_next_teacher_inputs is not None else nxt2
        return self._body(pc, nxt, labels, t_cur, t_nxt, False, nxt2, t_nxt2)


def _quiesce_process_groups(device, extra_groups=()):
    """Before a capture that will hold collectives.  What goes wrong otherwise (ROCm 7.0 / torch 2.10, seen in 1 of 7 runs
    on a 1-rank RCCL group, `Process group watchdog thread terminated with exception: HIP error: operation not permitted
    on an event last recorded in a capturing stream`): every process group's watchdog thread polls the end-events of the
    collectives issued EAGERLY on its RCCL stream (the warm-up steps' SyncBatchNorm exchanges and bucket all-reduces, the
    barrier below) until they have completed, once per 100 ms cycle.  The capture pulls those RCCL streams into capture
    mode, and HIP answers hipEventQuery on an event of a stream that has meanwhile entered capture with
    hipErrorCapturedEvent -- even though the event itself was recorded long before -- which the watchdog turns into a
    process abort.  So no eagerly issued collective may still sit in a watchdog's list when the capture begins: fence the
    ranks, complete everything on the device, then give every watchdog three of its cycles to retire the completed work.
    (Round 3 paused 1.5 s on a guess; the process-group API has no call that reports or drains that list.)"""
    import time
    dist.barrier()
    torch.cuda.synchronize(device)
    # Round 6: ProcessGroup._wait_for_pending_works() returns once the backend's list of issued-but-not-retired works -- the
    # very list the watchdog polls -- is empty: the condition itself instead of a pause long enough for it (three watchdog
    # cycles, 0.35 s, until round 5).  Every group that may hold such work: the default one and the ones created on top of it.
    waited = False
    try:
        groups = [dist.distributed_c10d._get_default_group()] + [g for g in extra_groups if g is not None]
        for g in groups:
            if hasattr(g, "_wait_for_pending_works"):
                g._wait_for_pending_works()
                waited = True
    except Exception:
        waited = False
    if not waited:
        time.sleep(0.35)                      # (no such call in this torch: the three-cycle pause)
    else:
        time.sleep(0.02)                      # the watchdog drops a retired work right after its query; let that pass finish
