"""Records what pointnet2/sa_fused.py ASKS of the library for one set-abstraction stage, without a device: the sequence of
C-ABI calls that `run` issues, forward and backward, on every value of every field of `StageRoute` and at the edges between
them.

    python tests/golden/make_golden_sa_calls.py [TREE [OUT.json]]

TREE is the checkout whose host code is the reference (default: the tree this file lies in), with its library built; the
table in this directory was recorded from the commit BEFORE the stage's hidden arguments (module globals, bare tuples, a plan
struct written halfway through its block) were made explicit, and tests/test_sa_stage_calls.py replays the cases on the tree
it runs in and compares exactly.

Nothing is launched.  The recorder stands one level below the one of make_golden_rows_calls.py: it replaces `_ext._run`, so the
`plan` argument that `sa_fused._call` appends for the plan-aware entry points is part of what is compared.  The zero pools
(`zeros_f32`, `zeros_f64`) are torch.zeros, so every tensor may live on the CPU (`torch.empty` never touches its memory: a
stage of 2^17 grouped rows costs nothing).  Only names that exist before and after are driven: `run`, `deferred_wgrads`,
`make_row_plan(into=)`, `build_csr_ahead`, `stage_route` and the module switches; a stage gets its ball-query indices from a
`chain_plan.StageAhead`, so no ball query runs.

Per call the recorder keeps what the rows recorder keeps (entry point, every int and float, per pointer "null" | "p" | "=k")
and, as the event's last entry, {"tag": `_ext.timing_tag` at the call (the stage label, forward and backward), "plan": for a
plan-aware entry point null or [rows, gs, pool_gamma set]}.  A `byref` scalar (the out-parameters of omnipq_gemm_tn_dz) is kept
as {"byref": value}, the layer records of omnipq_sa_infer as [ldw, C, eps, which pointers are set].  A case with `world`
replaces `_world` by that constant and `_allreduce_` by an "allreduce:<world>" event.  Every case ends with the deltas of the
`*_uses` counters.
"""
import contextlib
import ctypes
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _rows_generator():
    spec = importlib.util.spec_from_file_location("make_golden_rows_calls", os.path.join(HERE, "make_golden_rows_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rows_gen = _rows_generator()
USES = ("xyzgen_uses", "hoist_uses", "row_plan_uses", "last_no_dy_uses", "eval_chain_uses")


# ---- the cases ------------------------------------------------------------------------------------------------------
def _stage(npoint, nsample, mlp, route, **kw):
    """One PointnetSAModuleVotes(mlp=, npoint=, nsample=) on B scenes of N points.  mlp[0] = the feature channels (0: none).
    route: the fields of the StageRoute the stage must reach (asserted).  xyz_grad / feat_grad / w_grad: what requires a
    gradient; ahead: what arrives with the indices -- "" | "plan" | "plan+csr" (the CSR built under that plan) | "csr" (built
    over every row); chained: xyz and features are the previous stage's centres and output; label: omnipq_stage;
    sync: SyncBatchNorm layers."""
    s = dict(npoint=npoint, nsample=nsample, mlp=list(mlp), route=route, B=2, N=4096, training=True, xyz_grad=False,
             feat_grad=False, w_grad=True, ahead="", chained=False, label=None, sync=False, radius=0.2, normalize_xyz=False)
    s.update(kw)
    return s


def _case(*stages, **kw):
    """backward (True); no_grad (run under torch.no_grad()); deferred (backward inside deferred_wgrads); world (see above);
    switches {name in sa_fused: value}"""
    c = dict(stages=list(stages), backward=True, no_grad=False, deferred=False, world=None, switches={})
    c.update(kw)
    return c


PLANNED = dict(plan_gs=8, plan_arrives=False)
XYZ = [0, 64, 64, 128]            # 2^17 grouped rows at npoint 1024, nsample 64: planned, generated first layer
NO_DY = [0, 64, 128, 128]         # ... with c2 % 128 == 0, c3 % 128 == 0, c3 <= 256
F6 = [6, 64, 64, 128]             # six feature channels travel as eight: padded weight columns
F32 = [32, 64, 64, 128]           # features the first layer can run on at the source points


def cases():
    """[(name, case)], each named after the StageRoute values it reaches"""
    big = lambda mlp, route, **kw: _stage(1024, 64, mlp, route, **kw)
    small = lambda mlp, route, **kw: _stage(64, 32, mlp, route, **kw)                 # 4096 rows: the direct-atomics paths
    out = [
        # first layer
        ("first=xyz", _case(big(XYZ, dict(first="xyz", extrema="one", last="ysel", feed=("yab", "yab"), **PLANNED)))),
        ("first=grouped/cin6", _case(big(F6, dict(first="grouped", extrema="one", last="ysel", **PLANNED), feat_grad=True))),
        ("first=grouped/two_layers", _case(big([0, 64, 128], dict(first="grouped", extrema="one", last="ysel", **PLANNED)))),
        ("first=source", _case(big(F32, dict(first="source", extrema="one", last="ysel", **PLANNED), feat_grad=True))),
        ("first=source/hoist_off", _case(big(F32, dict(first="grouped", **PLANNED), feat_grad=True),
                                         switches={"HOIST_L1": False})),
        ("first=xyz/xyzgen_off", _case(big(XYZ, dict(first="grouped", **PLANNED)), switches={"XYZGEN": False})),
        ("first=chain", _case(_stage(256, 16, F32, dict(first="chain", feed=("lds", "lds"), finalize=("folded",) * 3),
                                     training=False), no_grad=True, backward=False)),
        ("first=chain/no_features", _case(_stage(256, 64, XYZ, dict(first="chain"), training=False, normalize_xyz=True,
                                                 radius=0.25), no_grad=True, backward=False)),
        ("eval/stored/grad_enabled", _case(_stage(256, 16, F32, dict(first="grouped", training=False,
                                                                     finalize=("running",) * 3), training=False),
                                           backward=False)),
        ("eval/stored/chain_off", _case(_stage(256, 16, XYZ, dict(first="grouped", training=False), training=False),
                                        no_grad=True, backward=False, switches={"EVAL_CHAIN": False})),
        # plan
        ("plan=none", _case(small(XYZ, dict(first="grouped", plan_gs=0, extrema="both", last="ysel")))),
        ("plan=none/row_plan_off", _case(big(XYZ, dict(first="xyz", plan_gs=0, extrema="both")),
                                         switches={"ROW_PLAN": False})),
        ("plan=forward/min_rows", _case(_stage(256, 32, XYZ, dict(first="xyz", extrema="one", **PLANNED)),
                                        switches={"PLAN_MIN_ROWS": 1 << 14})),
        ("plan=arrives", _case(big(XYZ, dict(first="xyz", plan_gs=8, plan_arrives=True, extrema="one"), ahead="plan"))),
        ("plan=arrives/no_dy", _case(big(NO_DY, dict(plan_gs=8, plan_arrives=True, last="no_dy"), ahead="plan"))),
        ("plan=arrives/csr_same_space", _case(big(F32, dict(first="source", plan_gs=8, plan_arrives=True),
                                                  ahead="plan+csr", feat_grad=True))),
        ("plan=arrives/csr_same_space/grouped", _case(big(F6, dict(first="grouped", plan_gs=8, plan_arrives=True),
                                                          ahead="plan+csr", feat_grad=True))),
        ("plan=forward/csr_other_space", _case(big(F32, dict(first="source", **PLANNED), ahead="csr", feat_grad=True))),
        ("plan=none/csr_other_space", _case(big(F32, dict(first="source", plan_gs=0, extrema="both"), ahead="plan+csr",
                                                feat_grad=True, xyz_grad=True))),
        ("plan=none/csr_same_space", _case(small(F32, dict(first="source", plan_gs=0), ahead="csr", feat_grad=True))),
        ("plan=forward/group16", _case(big(XYZ, dict(first="xyz", plan_gs=16, plan_arrives=False, extrema="both")),
                                       switches={"PLAN_GROUP": 16})),
        ("plan=arrives/group16", _case(big(NO_DY, dict(plan_gs=16, plan_arrives=True, extrema="both", last="no_dy"),
                                           ahead="plan"), switches={"PLAN_GROUP": 16})),
        # extrema
        ("extrema=none/pool_epilogue_off", _case(big(XYZ, dict(first="xyz", plan_gs=0, extrema="", last="y",
                                                               finalize=("consumer", "consumer", "launch"))),
                                                 switches={"POOL_EPILOGUE": False})),
        ("extrema=none/nsample48", _case(_stage(1024, 48, XYZ, dict(first="xyz", plan_gs=0, extrema="", last="y")))),
        ("extrema=none/small", _case(_stage(64, 48, F6, dict(first="grouped", plan_gs=0, extrema="", last="y"),
                                            feat_grad=True))),
        ("extrema=both", _case(big(XYZ, dict(first="xyz", extrema="both", **PLANNED)),
                               switches={"ONE_SIDED_EXTREMA": False})),
        ("extrema=one/two_layers/source", _case(big([32, 64, 128], dict(first="source", extrema="one", **PLANNED)))),
        # last
        ("last=y/small", _case(small(F6, dict(first="grouped", last="y", extrema=""), feat_grad=True),
                               switches={"POOL_EPILOGUE": False})),
        ("last=ysel/small", _case(small(F32, dict(first="source", last="ysel", extrema="both"), feat_grad=True))),
        ("last=no_dy", _case(big(NO_DY, dict(first="xyz", last="no_dy", keep_x2=True, extrema="one", **PLANNED)))),
        ("last=no_dy/last_x2_off", _case(big(NO_DY, dict(first="xyz", last="no_dy", keep_x2=False, **PLANNED)),
                                         switches={"LAST_X2": False})),
        ("last=no_dy/c3_256/source", _case(big([32, 128, 256], dict(first="source", last="no_dy", keep_x2=True, **PLANNED),
                                               feat_grad=True))),
        ("last=ysel/last_no_dy_off", _case(big(NO_DY, dict(first="xyz", last="ysel", **PLANNED)),
                                           switches={"LAST_NO_DY": False})),
        ("last=ysel/c3_512", _case(big([0, 64, 128, 512], dict(first="xyz", last="ysel", **PLANNED)))),
        # feed
        ("feed=stored", _case(big(XYZ, dict(first="grouped", plan_gs=0, feed=("stored", "stored"),
                                            finalize=("relu", "relu", "pool"), extrema="both", last="ysel")),
                              switches={"AFFINE_OPERANDS": False})),
        ("feed=stored/features", _case(small(F6, dict(first="grouped", feed=("stored", "stored")), feat_grad=True,
                                             xyz_grad=True), switches={"AFFINE_OPERANDS": False})),
        # gradients
        ("grad=xyz", _case(big(XYZ, dict(first="grouped", plan_gs=0, extrema="both", last="ysel"), xyz_grad=True))),
        ("grad=xyz/source", _case(big(F32, dict(first="source", plan_gs=0, extrema="both"), xyz_grad=True))),
        ("grad=xyz+features/cin6", _case(big(F6, dict(first="grouped", plan_gs=0), xyz_grad=True, feat_grad=True))),
        ("grad=features/source", _case(big(F32, dict(first="source", **PLANNED), feat_grad=True, normalize_xyz=True,
                                           radius=0.25))),
        ("grad=neither/source", _case(big(F32, dict(first="source", **PLANNED)))),
        ("grad=neither/cin6", _case(big(F6, dict(first="grouped", **PLANNED)))),
        ("grad=no_weights/source", _case(big(F32, dict(first="source", **PLANNED), feat_grad=True, w_grad=False))),
        ("grad=no_weights/cin6", _case(big(F6, dict(first="grouped", **PLANNED), feat_grad=True, w_grad=False))),
        ("grad=no_weights/no_dy", _case(big([32, 128, 128], dict(first="source", last="no_dy", **PLANNED), feat_grad=True,
                                            w_grad=False))),
    ]
    # weight gradients and collectives
    for name, st in (("xyz", big(XYZ, dict(first="xyz", **PLANNED))), ("no_dy", big(NO_DY, dict(last="no_dy", **PLANNED))),
                     ("source", big(F32, dict(first="source", **PLANNED), feat_grad=True)),
                     ("cin6", big(F6, dict(first="grouped", **PLANNED), feat_grad=True)),
                     ("small", small(F6, dict(first="grouped", plan_gs=0), feat_grad=True))):
        out.append(("deferred/" + name, _case(st, deferred=True)))
        out.append(("deferred/" + name + "/not_grouped", _case(st, deferred=True, switches={"SA_WGRADS_GROUPED": False})))
        out.append(("collectives/" + name, _case(st, switches={"_FORCE_COLLECTIVES": True})))
    out.append(("collectives/last=y", _case(small(F6, dict(first="grouped", last="y"), feat_grad=True),
                                            switches={"_FORCE_COLLECTIVES": True, "POOL_EPILOGUE": False})))
    # SyncBatchNorm layers, then plain BatchNorm2d layers, under a world of 2: only the first stage exchanges statistics
    for name, st in (("xyz", lambda **kw: big(XYZ, dict(first="xyz", **PLANNED), **kw)),
                     ("no_dy", lambda **kw: big(NO_DY, dict(last="no_dy", **PLANNED), **kw)),
                     ("small", lambda **kw: small(F6, dict(first="grouped", plan_gs=0), feat_grad=True, **kw))):
        out.append(("sync_then_plain/" + name, _case(st(sync=True), st(), world=2)))
    out.append(("sync/eval_chain", _case(_stage(256, 16, F32, dict(first="chain"), training=False, sync=True), world=2,
                                         no_grad=True, backward=False)))
    # two stages with labels of their own, the second fed by the first: both forwards before both backwards
    sa1 = big(XYZ, dict(first="xyz", **PLANNED), label="sa1")
    sa2 = _stage(256, 32, [128, 128, 128, 256], dict(first="source", plan_gs=0, extrema="both", last="ysel"), chained=True,
                 label="sa2", feat_grad=True)
    out.append(("labels/sa1_sa2", _case(sa1, sa2)))
    out.append(("labels/sa1_sa2/deferred", _case(sa1, sa2, deferred=True)))
    out.append(("labels/sa1_sa2/planned/deferred", _case(dict(sa1, mlp=NO_DY, route=dict(last="no_dy", **PLANNED)),
                                                         dict(sa2, route=dict(first="source", last="no_dy", **PLANNED)),
                                                         deferred=True, switches={"PLAN_MIN_ROWS": 1 << 14})))
    assert len({n for n, _ in out}) == len(out)
    return out


# ---- the recorder -----------------------------------------------------------------------------------------------------
_INFER_INTS = ("ldw", "C")
_INFER_PTRS = ("W", "gamma", "beta", "running_mean", "running_var")


class Recorder(rows_gen.Recorder):
    def __init__(self, ext):
        super().__init__()
        self.ext = ext

    def run(self, fn, anchor, *args):
        """in place of `_ext._run(fn, anchor, *args)`"""
        extra = {"tag": self.ext.timing_tag}
        if fn.__name__ in self.ext.PLAN_AWARE:
            *args, plan = args
            extra["plan"] = None if plan is None else [int(plan.contents.rows), int(plan.contents.gs),
                                                       int(bool(plan.contents.pool_gamma))]
        flat, special = [], {}
        for i, a in enumerate(args):
            obj = getattr(a, "_obj", None)
            if isinstance(obj, ctypes._SimpleCData):
                special[i] = {"byref": obj.value}
            elif isinstance(obj, ctypes.Array) and hasattr(obj._type_, "running_var"):
                special[i] = [[getattr(q, n) for n in _INFER_INTS] + [q.eps] + [int(bool(getattr(q, n))) for n in _INFER_PTRS]
                              for q in obj]
            flat.append(0 if i in special else a)
        self.call(fn, anchor, *flat)
        for i, value in special.items():
            self.events[-1][1 + i] = value
        self.events[-1].append(extra)


def _module(torch, st):
    import pointnet2_modules
    mod = pointnet2_modules.PointnetSAModuleVotes(mlp=list(st["mlp"]), npoint=st["npoint"], radius=st["radius"],
                                                  nsample=st["nsample"], normalize_xyz=st["normalize_xyz"])
    if st["sync"]:
        mod = torch.nn.SyncBatchNorm.convert_sync_batchnorm(mod)
    if st["label"]:
        mod.omnipq_stage = st["label"]
    mod.train(st["training"])
    for p in mod.parameters():
        if p.dim() > 1:
            p.requires_grad_(st["w_grad"])
    return mod


def _ahead(torch, sa_fused, st, idx, N):
    """the chain_plan.StageAhead of the stage: its indices and what was made ahead of it"""
    import chain_plan
    B, M, S = idx.shape
    P = B * M * S
    state, plan, csr = None, None, None
    if "plan" in st["ahead"]:
        state = torch.zeros(sum(sa_fused.plan_words(B, M, P)), dtype=torch.int32)
        plan = sa_fused.make_row_plan(idx, P, into=state)
    if "csr" in st["ahead"]:
        offsets, order = torch.zeros(B, N + 1, dtype=torch.int32), torch.zeros(B, M * S, dtype=torch.int32)
        sa_fused.build_csr_ahead(idx, N, plan, offsets, order)
        csr = chain_plan.Csr(offsets, order, None if plan is None else (state.data_ptr(), plan.gs))
    return chain_plan.StageAhead(None, idx, state, csr, None, plan is not None)


def run_case(case):
    """-> the events of one case, forward then (after "backward") backward, then {"uses": the counters' deltas}"""
    import torch
    import sa_fused
    ext = sa_fused._ext
    rec = Recorder(ext)
    patches = [(ext, "_run", rec.run),
               (sa_fused, "zeros_f32", lambda n, device: torch.zeros(n)),
               (sa_fused, "zeros_f64", lambda rows, cols, device: torch.zeros(rows, cols, dtype=torch.float64))]
    if case["world"] is not None:
        def exchange(sums, world=None):
            if (case["world"] if world is None else world) > 1:
                rec.events.append("allreduce:%d" % (case["world"] if world is None else world))
            return sums
        patches += [(sa_fused, "_world", lambda: case["world"]), (sa_fused, "_allreduce_", exchange)]
    patches += [(sa_fused, name, value) for name, value in case["switches"].items()]
    torch.manual_seed(0)
    grad = torch.no_grad() if case["no_grad"] else torch.enable_grad()
    block = sa_fused.deferred_wgrads() if case["deferred"] else contextlib.nullcontext()
    outs, prev = [], None
    with rows_gen._patched(patches), grad:
        before = [getattr(sa_fused, n) for n in USES]
        for st in case["stages"]:
            mod = _module(torch, st)
            B, M, S = st["B"], st["npoint"], st["nsample"]
            if st["chained"]:
                xyz, features = prev
            else:
                xyz = torch.empty(B, st["N"], 3).requires_grad_(st["xyz_grad"])
                features = torch.empty(B, st["mlp"][0], st["N"]).requires_grad_(st["feat_grad"]) if st["mlp"][0] else None
            N = xyz.shape[1]
            new_xyz = torch.empty(B, M, 3)
            idx = torch.zeros(B, M, S, dtype=torch.int32)
            group = _ahead(torch, sa_fused, st, idx, N)
            # the route the case is named after, from the same pure function the stage asks (a case cannot drift to another)
            widths = [layer.conv.out_channels for layer in mod.mlp_module]
            arrives = group.plan_state is not None
            route = sa_fused.stage_route(
                st["training"], B, N, M, S, st["mlp"][0], widths, features is not None,
                bool(not case["no_grad"] and xyz.requires_grad),
                bool(not case["no_grad"] and features is not None and features.requires_grad),
                sa_fused.PLAN_GROUP if arrives else None, arrives, no_grad=case["no_grad"])
            for field, value in st["route"].items():
                assert getattr(route, field) == value, (field, getattr(route, field), value, route)
            out = sa_fused.run(mod, xyz, new_xyz, features, group=group)
            outs.append(out)
            prev = (new_xyz, out)
        if case["backward"]:
            rec.events.append("backward")
            with block:
                torch.autograd.backward(outs[-1:] if case["stages"][-1]["chained"] else outs,
                                        [torch.ones_like(o) for o in (outs[-1:] if case["stages"][-1]["chained"] else outs)])
        rec.events.append({"uses": [getattr(sa_fused, n) - b for n, b in zip(USES, before)]})
    return rec.events


def record():
    """-> {"events": [distinct events], "sequences": [distinct lists of event numbers], "cases": [[name, sequence number]]}"""
    events, sequences, table = {}, {}, []
    for name, case in cases():
        seq = tuple(events.setdefault(json.dumps(ev), len(events)) for ev in run_case(case))
        table.append([name, sequences.setdefault(seq, len(sequences))])
    return {"events": [json.loads(e) for e in events], "sequences": [list(s) for s in sequences], "cases": table}


expand = rows_gen.expand


if __name__ == "__main__":
    tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "sa_stage_calls.json")
    pkg = os.path.join(tree, "omni-pq_amd")
    for p in (pkg, os.path.join(pkg, "pointnet2"), os.path.join(pkg, "models")):
        sys.path.insert(0, p)
    table = record()
    with open(out, "w") as fh:
        fh.write("{\n\"events\": [\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in table["events"]))
        fh.write("\n],\n\"sequences\": [\n" + ",\n".join(json.dumps(s, separators=(",", ":")) for s in table["sequences"]))
        fh.write("\n],\n\"cases\": [\n" + ",\n".join(json.dumps(c) for c in table["cases"]) + "\n]\n}\n")
    print(f"{out}: {len(table['cases'])} cases, {len(table['sequences'])} sequences, {len(table['events'])} events")
