"""Captured inference: the eval forward and the packed detections of a batch as ONE replayed graph, one readback per record.

    runner = CapturedInference(net, example_inputs, config_dict)
    for batch, nxt in train_step.lookahead(loader):
        dets = runner.run(batch, next_inputs=nxt)            # {prefix: (Detections | None, quad Detections | None)}
        boxes, quads = dets["last_"]
        batch_pred_map_cls, pred_mask = boxes.to_lists()      # what ap_helper_pq.parse_predictions returns
        ...

The eval / no_grad forward is host-bound (what is timed is the host enqueueing launches), and what follows it
in the evaluation loop -- parse_predictions, parse_quad_predictions -- is some 25 small launches and 9 synchronising copies per
prefix.  The body captured here is the forward under no_grad and autocast, with the sampling chain of the NEXT batch started
inside it (net.prefetch(..., at_next_forward=True), as train_step.CapturedStep does), followed by
ap_helper_pq.detect_predictions / detect_quad_predictions with `out=`: no host read, no allocation outside the graph's pool.
`run` copies the batch into the static input, replays, and then issues the records' device-to-host copies
(Detections.to_host) eagerly on the same stream: they stay OUTSIDE the graph, which therefore holds kernel nodes only.

The thresholds and modes of `config_dict` are launch ARGUMENTS of the captured kernels and so are fixed at capture: a changed
config needs a new runner, and `run` raises when it finds the dict's scalars (or the dataset config's class counts and mean
sizes) changed.  One rank only: multi-GPU evaluation is independent runners.

    scorer = evaluate_layout_f1(runner, batches)              # batches: dicts of point_clouds and the quad labels, on the device
    f1 = scorer.f1(calculated=True)                           # the first host read of the pass: five integers

is the evaluation pass that ends in the layout F1: every batch is run with `to_host=False` and its quad record is
scored on the device (ap_helper_pq.LayoutF1), so no record is copied and no Python list is built.
"""
import gc

import numpy as np
import torch

from train_step import _cloud, lookahead


def _config_snapshot(config_dict):
    """the part of config_dict that became launch arguments, as something `==` compares"""
    snap = {k: v for k, v in config_dict.items() if isinstance(v, (bool, int, float, str, type(None)))}
    dc = config_dict.get("dataset_config")
    if dc is not None:
        snap["dataset_config"] = (id(dc), int(dc.num_class), int(dc.num_heading_bin),
                                  np.asarray(dc.mean_size_arr, dtype=np.float64).tobytes())
    return snap


class CapturedInference:
    """runner = CapturedInference(net, example_inputs, config_dict, *, amp_dtype=torch.bfloat16, graph=True,
                                  prefetch="forward", prefixes=("last_",), objects=True, quads=True, warmup=3)

    net              the bare PQ_Transformer in eval mode (net.eval()); a net in train mode is refused.
    example_inputs   {'point_clouds': (B, N, 3 + C) f32 on the GPU} (or the tensor): fixes the batch shape; its contents are
                     only used for the warm-up runs.
    config_dict      what parse_predictions / parse_quad_predictions take.  Fixed at construction (see the module text).
    amp_dtype        torch.bfloat16 / torch.float16 / None (strict f32).
    graph            True: capture once, replay per batch.  False: the identical body launched eagerly on the caller's
                     tensors -- the debugging and A/B route, and the fallback.
    prefetch         "forward": the coordinate-only sampling of `next_inputs` starts inside this batch's forward and runs
                     underneath it.  None: every forward samples its own batch.
    prefixes         the stages whose predictions are packed ("last_", "0head_", ..., "proposal_").
    objects, quads   which of the two records to make per prefix.

    runner.run(inputs, next_inputs=None) -> {prefix: (Detections | None, quad Detections | None)}: the runner's own records,
    rewritten by the next run(); their to_host() copies are already queued, so to_lists() only waits for them.
    runner.end_points: the (static, detached) outputs of the forward.  runner.launch: "hipGraph replay" | "eager".
    The sampling plan of an announced batch lives in buffers of `net`: if anything else runs a forward of `net` between two
    run() calls, call runner.forget_next() before the next one.
    """

    def __init__(self, net, example_inputs, config_dict, *, amp_dtype=torch.bfloat16, graph=True, prefetch="forward",
                 prefixes=("last_",), objects=True, quads=True, warmup=3):
        if net.training:
            raise RuntimeError("CapturedInference: the network is in train mode -- call net.eval() first (BatchNorm would "
                               "normalise with, and update, batch statistics, and dropout would be live)")
        if prefetch not in ("forward", None):
            raise ValueError('CapturedInference: prefetch is "forward" or None')
        if not (objects or quads) or not prefixes:
            raise ValueError("CapturedInference: nothing to detect (objects, quads and prefixes)")
        self.net, self.config, self.amp_dtype = net, config_dict, amp_dtype
        self.prefetch_at = prefetch
        self.prefixes, self.objects, self.quads = tuple(prefixes), bool(objects), bool(quads)
        self._snapshot = _config_snapshot(config_dict)
        pc = _cloud(example_inputs)
        self.cur, self.nxt = pc.clone(), pc.clone()
        self.records = {p: (None, None) for p in self.prefixes}
        self.end_points = None
        self.graph = None
        self.launch = "eager"
        self.replays = 0
        self._promised = None          # the tensor announced as `next_inputs` by the previous call (kept alive: compared with `is`)
        self._have_next = False        # does `nxt` (and the plan in flight) hold the batch the next call will run?
        if graph:
            self._capture(warmup)

    # ---- what is captured --------------------------------------------------------------------------------------------------
    _capturing = False

    def _body(self, cur, nxt, trusted):
        """forward of `cur` with the sampling plan of `nxt` started inside it, then the packed detections of every prefix
        into the runner's records"""
        import ap_helper_pq
        net = self.net
        if self.prefetch_at == "forward" and nxt is not None:
            net.prefetch({"point_clouds": nxt}, trusted=trusted, at_next_forward=True)
        with torch.no_grad(), torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype is not None):
            ep = net({"point_clouds": cur})
        if self._capturing:
            net.join_prefetch()                      # the sampling stream joins before the capture ends
        self.end_points = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in ep.items()}
        ep = dict(self.end_points)
        ep.setdefault("point_clouds", cur)           # remove_empty_box counts the scene's points
        for prefix in self.prefixes:
            boxes, quads = self.records[prefix]
            if self.objects:
                boxes = ap_helper_pq.detect_predictions(ep, self.config, prefix, out=boxes)
            if self.quads:
                quads = ap_helper_pq.detect_quad_predictions(ep, self.config, prefix, out=quads)
            self.records[prefix] = (boxes, quads)
        return self.records

    def _capture(self, warmup):
        import sa_fused
        net = self.net
        self._capturing = True
        try:
            self.nxt.copy_(self.cur)
            if self.prefetch_at is not None:
                net.prefetch({"point_clouds": self.nxt}, trusted=True)          # plan of the first batch
            for _ in range(max(int(warmup), 3)):     # eager warm-up: allocator pools, workspaces, weight arenas, the records
                self.cur.copy_(self.nxt)
                self._body(self.cur, self.nxt if self.prefetch_at else None, True)
            torch.cuda.synchronize()
            sa_fused.reset_pools()
            # A captured graph that died in a reference cycle (an earlier runner or CapturedStep) must not be collected inside
            # this capture: on ROCm its destructor synchronises the device, which a capture in progress refuses
            # (train_step.CapturedStep._capture).
            gc.collect()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._body(self.cur, self.nxt if self.prefetch_at else None, True)
            self.graph = graph
            self.launch = "hipGraph replay"
            self._have_next = self.prefetch_at is not None      # `nxt` holds the example batch, the capture run started its plan
            net.forget_prefetch()
        finally:
            self._capturing = False

    # ---- one batch ---------------------------------------------------------------------------------------------------------
    def _check(self):
        if self.net.training:
            raise RuntimeError("CapturedInference.run: the network was put back into train mode -- call net.eval()")
        if _config_snapshot(self.config) != self._snapshot:
            raise RuntimeError("CapturedInference.run: config_dict changed since the runner was built; its thresholds and "
                               "modes are launch arguments fixed at capture -- build a new runner for a new config")

    def run(self, inputs=None, next_inputs=None, to_host=True):
        """Detections of `inputs`.  next_inputs: the batch the NEXT call will run (tensor / dict / callable(dst) filling the
        static buffer): its sampling runs underneath this forward.  inputs=None, or the very object announced as
        `next_inputs` by the previous call: the announced batch is taken as is; any other input is copied in and, with
        prefetch="forward", sampled in front of the replay.  to_host=False: the records' to_host() copies are not queued
        (their pinned twins keep what the last copy left): for a consumer that stays on the device (evaluate_layout_f1)."""
        self._check()
        if self.graph is None:
            return self._finish(self._eager(inputs, next_inputs), to_host)
        net = self.net
        pc = None if inputs is None else _cloud(inputs)
        announced = self._have_next and (pc is None or (self._promised is not None and self._promised[0] is pc
                                                        and self._promised[1] == pc._version))
        if announced:
            self.cur.copy_(self.nxt)
        else:
            if pc is None:
                raise ValueError("CapturedInference.run: no batch was announced by the previous call; pass `inputs`")
            self.cur.copy_(pc)
            if self.prefetch_at is not None:
                # the plan in flight belongs to some other batch: sample this one now, ahead of the replay
                net.prefetch({"point_clouds": self.cur}, trusted=True)
                net.join_prefetch()
        if self.prefetch_at is not None and next_inputs is not None:
            if callable(next_inputs):
                next_inputs(self.nxt)
                self._promised = None
            else:
                t = _cloud(next_inputs)
                self.nxt.copy_(t)
                self._promised = (t, t._version)     # the object itself, kept alive until the next call: an address can be reused
            self._have_next = True
        else:
            self._promised, self._have_next = None, False
        self.graph.replay()
        self.replays += 1
        net.forget_prefetch()            # the replayed graph owns the sampling chain; no later eager forward may take its plan
        return self._finish(self.records, to_host)

    def forget_next(self):
        """Call after anything else ran a forward of `net` (another runner, a plain evaluation pass): that forward reused the
        sampling chain's buffers, so the plan of the batch announced by the last run() is gone.  The next run() then takes
        its `inputs` as unannounced and samples them in front of the replay."""
        self._promised, self._have_next = None, False
        self.net.forget_prefetch()

    def _eager(self, inputs, next_inputs):
        if inputs is None:
            raise ValueError("CapturedInference.run (eager): pass `inputs`")
        nxt = None
        if next_inputs is not None and not callable(next_inputs) and self.prefetch_at is not None:
            nxt = _cloud(next_inputs)
        return self._body(_cloud(inputs), nxt, False)

    @staticmethod
    def _finish(records, to_host=True):
        if not to_host:
            return records
        for boxes, quads in records.values():
            for det in (boxes, quads):
                if det is not None:
                    det.to_host()                # eagerly, behind the replay on the same stream: no memcpy node in the graph
        return records


def evaluate_layout_f1(runner, batches, prefix="last_"):
    """The layout F1 of an evaluation pass without a host read per batch: -> ap_helper_pq.LayoutF1.

    batches: an iterable of dicts holding `point_clouds` and the quad labels on the device (gt_quad_centers,
    gt_normal_vectors, gt_quad_sizes, num_total_quads, horizontal_quads -- what device_data.DeviceLoader assembles).  Every
    batch is run with the following one announced and to_host=False, and its quad record of `prefix` is scored where it is
    (LayoutF1.step: two launches).  Nothing is read until the caller asks the returned scorer: .read() / .f1(calculated)."""
    import ap_helper_pq
    if not runner.quads or prefix not in runner.prefixes:
        raise ValueError(f"evaluate_layout_f1: the runner packs no quad record for prefix {prefix!r}")
    scorer = ap_helper_pq.LayoutF1(runner.cur.device)
    for batch, nxt in lookahead(batches):
        quads = runner.run(batch, next_inputs=nxt, to_host=False)[prefix][1]
        scorer.step(quads, batch)
    return scorer
