"""Records what pointnet2/rows_mlp.py ASKS of the library, without a device: the sequence of C-ABI calls that `run` and
`run_pair` issue, forward and backward, for the stacks the model runs and for the edges of every route.

    python tests/golden/make_golden_rows_calls.py [TREE [OUT.json]]

TREE is the checkout whose host code is the reference (default: the tree this file lies in), with its library built; the
table in this directory was recorded from the commit BEFORE the rows engine's routes were put into `stack_route()`, and
tests/test_rows_mlp_calls.py replays the cases on the tree it runs in and compares exactly.

Nothing is launched: `_call` of rows_mlp and of sa_fused is replaced by the recorder, the zero pools (`zeros_f32` in both
modules, `zeros_f64` in sa_fused) by torch.zeros, and `rows_mlp._hold` by an event, so every tensor may live on the CPU.
Only those names and module switches are patched.  Per call the recorder keeps the entry point's name, every int and float
argument, and for every pointer `"null"`, `"p"`, or `"=k"`: the same address as argument k of this call (an in-place pass).
Of a grouped weight-gradient launch it keeps every problem's integers and which of its pointers are set.
"""
import contextlib
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

# ---- the cases ------------------------------------------------------------------------------------------------------
# A stack: (cin, ((cout, kind), ...), rows) with kind "bn" (linear + BatchNorm + ReLU) | "act" (linear + ReLU + dropout) |
# "plain"; options: bias (default True), f32 (the input's dtype: the coordinates of the position embeddings), cat (the last
# layer's weight and bias are a cat_params of three parts: the output heads of a prediction head).
LIN864 = (288, ((864, "plain"),), 300)
LIN576 = (288, ((576, "plain"),), 1000)
LIN288 = (288, ((288, "plain"),), 300)
FF = (288, ((2048, "act"), (288, "plain")), 300)
POS = (3, ((288, "bn"), (288, "plain")), 1000, {"f32": True})
VOTE = (288, ((288, "bn"), (288, "bn"), (291, "plain")), 2048)
HEAD = (288, ((288, "bn"), (288, "bn"), (97, "plain")), 300)
HEAD_CAT = (288, ((288, "bn"), (288, "bn"), (97, "plain")), 300, {"cat": True})
FP = (1024, ((512, "bn"), (512, "bn")), 1000, {"bias": False})
K1024 = (1024, ((64, "act"), (32, "plain")), 300)                  # an act layer with a contraction of 1024
BELOW1024 = (96, ((256, "act"), (1024, "plain")), 300)             # an act layer below a layer 1024 wide
ACT_ON_BN = (96, ((128, "bn"), (256, "act"), (64, "plain")), 300)  # an act layer fed from (Y, a, b)
HUGE = (32, ((2048, "act"), (32, "plain")), 1 << 21)               # rows * width = 2^32 (forward only: nothing is touched)
PAIR_A = (288, ((288, "bn"), (288, "bn"), (128, "plain")), 300)
PAIR_B = (288, ((288, "bn"), (288, "bn"), (32, "plain")), 300)
DEEP = (288, ((288, "bn"), (288, "bn"), (97, "plain")), 2048)
SHALLOW = (288, ((288, "bn"), (288, "plain")), 1000)
STACKS = {"lin864": LIN864, "lin576": LIN576, "lin288": LIN288, "ff": FF, "pos": POS, "vote": VOTE, "head": HEAD,
          "head_cat": HEAD_CAT, "fp": FP}
BN_LESS = ("lin864", "lin576", "lin288", "ff")
FUSE_ACT, AFFINE, FORCE = ("rows_mlp", "_FUSE_ACT"), ("sa_fused", "AFFINE_OPERANDS"), ("sa_fused", "_FORCE_COLLECTIVES")


def _case(stacks, **kw):
    """training (True), backward (True: with gradients), in_grad (True: the input needs one), p (dropout of act layers),
    padded, use (which outputs of a pair reach the loss), same_input (a pair over ONE input tensor), deferred (inside
    deferred_wgrads), switches ({(module, name): value})"""
    c = dict(stacks=stacks, training=True, backward=True, in_grad=True, p=0.0, padded=False, use=(True, True),
             same_input=False, deferred=False, switches={})
    c.update(kw)
    return c


def _lone_and_pairs():
    """cases 1 and 3 of the table: run as they are, inside deferred_wgrads, and with the collectives forced"""
    out = []
    for name, st in STACKS.items():
        out.append((name, _case([st])))
        out.append((name + "/no_in_grad", _case([st], in_grad=False)))
    out.append(("ff/p", _case([FF], p=0.1)))
    out.append(("ff/p/no_in_grad", _case([FF], p=0.1, in_grad=False)))
    out.append(("vote/padded", _case([VOTE], padded=True)))
    out.append(("pair/equal", _case([PAIR_A, PAIR_B])))
    out.append(("pair/equal/no_in_grad", _case([PAIR_A, PAIR_B], in_grad=False)))
    out.append(("pair/unequal", _case([DEEP, SHALLOW])))
    out.append(("pair/unequal/swapped", _case([SHALLOW, DEEP])))
    out.append(("pair/only_a_used", _case([PAIR_A, PAIR_B], use=(True, False))))
    out.append(("pair/only_b_used", _case([PAIR_A, PAIR_B], use=(False, True))))
    out.append(("pair/same_input", _case([POS, POS], same_input=True, in_grad=False)))
    out.append(("pair/lin", _case([LIN288, LIN288])))
    out.append(("pair/head_cat", _case([HEAD_CAT, PAIR_B])))
    return out


def cases():
    """[(name, case)]"""
    out = _lone_and_pairs()
    for name, st in STACKS.items():
        out.append((name + "/eval", _case([st], training=False, backward=False)))
    for name in BN_LESS:
        out.append((name + "/eval_grad", _case([STACKS[name]], training=False)))
    out.append(("pair/equal/eval", _case([PAIR_A, PAIR_B], training=False, backward=False)))
    # the edges of the routes, and each switch off
    for name, st in (("k1024", K1024), ("below1024", BELOW1024), ("act_on_bn", ACT_ON_BN)):
        out.append((name, _case([st], p=0.5)))
        out.append((name + "/p0", _case([st])))
    out.append(("huge/forward", _case([HUGE], p=0.5, backward=False)))
    for name, st, p in (("ff", FF, 0.0), ("ff/p", FF, 0.1), ("k1024", K1024, 0.5), ("below1024", BELOW1024, 0.5),
                        ("act_on_bn", ACT_ON_BN, 0.5)):
        out.append((name + "/no_fuse_act", _case([st], p=p, switches={FUSE_ACT: False})))
    out.append(("ff/eval_grad/no_fuse_act", _case([FF], training=False, switches={FUSE_ACT: False})))
    for name in ("pos", "vote", "head", "fp"):
        out.append((name + "/no_affine", _case([STACKS[name]], switches={AFFINE: False})))
    out.append(("act_on_bn/no_affine", _case([ACT_ON_BN], p=0.5, switches={AFFINE: False})))
    out.append(("pair/equal/no_affine", _case([PAIR_A, PAIR_B], switches={AFFINE: False})))
    out.append(("pair/unequal/no_affine", _case([DEEP, SHALLOW], switches={AFFINE: False})))
    for name, c in _lone_and_pairs():
        out.append((name + "/deferred", dict(c, deferred=True)))
    for name, c in _lone_and_pairs():
        out.append((name + "/collectives", dict(c, switches={FORCE: True})))
    out.append(("pair/equal/collectives/no_affine", _case([PAIR_A, PAIR_B], switches={FORCE: True, AFFINE: False})))
    out.append(("pair/equal/collectives/deferred", _case([PAIR_A, PAIR_B], switches={FORCE: True}, deferred=True)))
    assert len({n for n, _ in out}) == len(out)
    return out


# ---- the recorder -----------------------------------------------------------------------------------------------------
_PROBLEM_INTS = ("M", "N", "P", "lda", "ldb", "out_rows", "out_cols", "out_ld", "flags", "rot")
_PROBLEM_PTRS = ("A", "B", "colsum", "out", "ba", "bb", "rows_dev")


class Recorder:
    def __init__(self):
        self.events = []

    def call(self, fn, anchor, *args):
        ev, seen = [fn.__name__], {}
        for i, a in enumerate(args):
            if isinstance(a, ctypes.c_void_p):
                addr = a.value or 0
                ev.append("null" if not addr else "=%d" % seen[addr] if addr in seen else "p")
                if addr:
                    seen.setdefault(addr, i)
            elif isinstance(a, (bool, int)):
                ev.append(int(a))
            elif isinstance(a, float):
                ev.append(a)
            elif hasattr(a, "_obj"):                 # byref(array of omnipq_tn_problem): the grouped weight gradients
                ev.append([[getattr(q, n) for n in _PROBLEM_INTS] + [int(bool(getattr(q, n))) for n in _PROBLEM_PTRS]
                           for q in a._obj])
            else:
                raise TypeError(f"{fn.__name__}: argument {i} of type {type(a).__name__} is not recorded")
        self.events.append(ev)

    def hold(self, lead):
        self.events.append("hold:%d" % bool(lead))


@contextlib.contextmanager
def _patched(pairs):
    saved = [(mod, name, getattr(mod, name)) for mod, name, _ in pairs]          # (a missing name raises: nothing is added)
    try:
        for mod, name, value in pairs:
            setattr(mod, name, value)
        yield
    finally:
        for mod, name, value in reversed(saved):
            setattr(mod, name, value)


def _build(torch, rows_mlp, sa_fused, st, p):
    cin, layers, n = st[:3]
    opt = st[3] if len(st) > 3 else {}
    out, c = [], cin
    for i, (cout, kind) in enumerate(layers):
        if opt.get("cat") and i == len(layers) - 1:
            third = cout // 3
            parts = (third, cout - 2 * third, third)
            w = sa_fused.cat_params([torch.nn.Parameter(torch.zeros(q, c, 1)) for q in parts])
            b = sa_fused.cat_params([torch.nn.Parameter(torch.zeros(q)) for q in parts], pad_to=(cout + 31) // 32 * 32)
        else:
            w = torch.nn.Parameter(torch.zeros(cout, c, 1) if kind == "bn" else torch.zeros(cout, c))
            b = torch.nn.Parameter(torch.zeros(cout)) if opt.get("bias", True) else None
        out.append(rows_mlp.Layer(w, b, bn=torch.nn.BatchNorm1d(cout) if kind == "bn" else None,
                                  relu_dropout=p if kind == "act" else None))
        c = cout
    return out


def run_case(case):
    """-> the events of one case, forward then (after "backward") backward"""
    import torch
    import dropout_state
    import rows_mlp
    import sa_fused
    mods = {"rows_mlp": rows_mlp, "sa_fused": sa_fused}
    rec = Recorder()
    patches = [(rows_mlp, "_call", rec.call), (sa_fused, "_call", rec.call), (rows_mlp, "_hold", rec.hold),
               (rows_mlp, "zeros_f32", lambda n, device: torch.zeros(n)),
               (sa_fused, "zeros_f32", lambda n, device: torch.zeros(n)),
               (sa_fused, "zeros_f64", lambda rows, cols, device: torch.zeros(rows, cols, dtype=torch.float64))]
    patches += [(mods[m], name, value) for (m, name), value in case["switches"].items()]
    torch.manual_seed(0)
    dropout_state.STATE.reset()                      # the salts restart at 1 in every case
    stacks = [_build(torch, rows_mlp, sa_fused, st, case["p"]) for st in case["stacks"]]
    xs = []
    for st in case["stacks"]:
        f32 = len(st) > 3 and st[3].get("f32")
        xs.append(torch.empty(st[2], st[0], dtype=torch.float32 if f32 else torch.bfloat16))
    if case["same_input"]:
        xs[1] = xs[0]
    if case["in_grad"]:
        xs = [x.requires_grad_(True) for x in xs]
    grad = torch.enable_grad() if case["backward"] else torch.no_grad()
    block = sa_fused.deferred_wgrads() if case["deferred"] else contextlib.nullcontext()
    with _patched(patches), grad:
        if len(stacks) == 1:
            ys = [rows_mlp.run(xs[0], stacks[0], case["training"], padded=case["padded"])]
        else:
            ys = rows_mlp.run_pair(xs[0], stacks[0], xs[1], stacks[1], case["training"], padded=case["padded"])
        if case["backward"]:
            rec.events.append("backward")
            used = [y for y, u in zip(ys, case["use"]) if u]
            with block:
                torch.autograd.backward(used, [torch.ones_like(y) for y in used])
    return rec.events


def record():
    """-> {"events": [distinct events], "sequences": [distinct lists of event numbers], "cases": [[name, sequence number]]}"""
    events, sequences, table = {}, {}, []
    for name, case in cases():
        seq = tuple(events.setdefault(json.dumps(ev), len(events)) for ev in run_case(case))
        table.append([name, sequences.setdefault(seq, len(sequences))])
    return {"events": [json.loads(e) for e in events], "sequences": [list(s) for s in sequences], "cases": table}


def expand(table):
    """{case name: its events}"""
    return {name: [table["events"][i] for i in table["sequences"][s]] for name, s in table["cases"]}


if __name__ == "__main__":
    tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "rows_mlp_calls.json")
    pkg = os.path.join(tree, "omni-pq_amd")
    for p in (pkg, os.path.join(pkg, "pointnet2"), os.path.join(pkg, "models")):
        sys.path.insert(0, p)
    table = record()
    with open(out, "w") as fh:
        fh.write("{\n\"events\": [\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in table["events"]))
        fh.write("\n],\n\"sequences\": [\n" + ",\n".join(json.dumps(s, separators=(",", ":")) for s in table["sequences"]))
        fh.write("\n],\n\"cases\": [\n" + ",\n".join(json.dumps(c) for c in table["cases"]) + "\n]\n}\n")
    print(f"{out}: {len(table['cases'])} cases, {len(table['sequences'])} sequences, {len(table['events'])} events")
