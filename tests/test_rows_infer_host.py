"""CPU (needs the built libraries, no GPU): the host side of the inference stack kernel (csrc/rows_infer.hip) -- which route
rows_mlp.stack_route gives an eval stack with and without `no_grad`, the predicate that asks the library for its limits, the
argument checks of omnipq_rows_infer that run before anything is launched, the calls the opted-in forward issues (with the
recorder of tests/golden/make_golden_rows_calls.py), and the three new symbols' declarations."""
import ctypes
import json
import os
import sys

import pytest
import torch

import capi
import rows_infer_reference as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_rows_calls as G  # noqa: E402

EINVAL = 10001
# name: (rows, cin, layers): the stacks the model's eval forward runs (tests/golden/make_golden_rows_calls.py) and its FP shapes
MODEL = {"pos": (1000, 3, ((288, "bn"), (288, "plain"))),
         "pos6": (2048, 6, ((288, "bn"), (288, "plain"))),
         "vote": (2048, 288, ((288, "bn"), (288, "bn"), (291, "plain"))),
         "head": (300, 288, ((288, "bn"), (288, "bn"), (97, "plain"))),
         "fp-golden": (1000, 1024, ((512, "bn"), (512, "bn"))),
         "fp1": (4096, 1024, ((512, "bn"), (512, "bn"))),
         "fp2": (8192, 1024, ((512, "bn"), (288, "bn"))),
         "act-on-bn": (300, 96, ((128, "bn"), (256, "act"), (64, "plain")))}
# stacks the chain does not take, whatever the mode: no hidden layer; a layer wider than 640 (the feed-forward block); an
# input wider than 1024; four layers; a BatchNorm width that is no multiple of 32
NOT_TAKEN = {"one layer": (300, 288, ((864, "plain"),)),
             "the feed-forward block": (300, 288, ((2048, "act"), (288, "plain"))),
             "an input of 1056 channels": (300, 1056, ((64, "bn"), (32, "plain"))),
             "four layers": (300, 32, ((64, "bn"), (64, "bn"), (64, "bn"), (32, "plain"))),
             "a BatchNorm of 48 channels": (300, 32, ((48, "bn"), (32, "plain")))}
# (kpad, widths) the kernel does not take, one per rule of include/omnipq_decoder.h
REFUSED = {"a width of 48": (32, (64, 48, 64)), "a width of 0": (32, (64, 0)), "four layers": (32, (64, 64, 64, 64)),
           "a width of 672": (32, (64, 672, 64)), "no layer": (32, ()), "kpad % 32": (48, (64, 64)), "kpad of 0": (0, (64,)),
           "kpad above 1024": (1056, (64, 64))}
TAKEN = {"one layer": (32, (64,)), "the widest": (1024, (640, 640, 640)), "1024 -> 512 -> 512": (1024, (512, 512)),
         "head": (288, (288, 288, 128))}


def _lds_bytes(lib, kpad, widths):
    lib.omnipq_rows_infer_lds_bytes.restype = ctypes.c_longlong
    arr = (ctypes.c_int * max(len(widths), 1))(*widths)
    return int(lib.omnipq_rows_infer_lds_bytes(kpad, len(widths), arr))


def _chain(layers):
    import rows_mlp
    return rows_mlp.StackRoute(False, tuple(
        rows_mlp.LayerRoute(kind, "lds" if l else "input", "chain", "folded" if kind == "bn" else "",
                            "epilogue" if kind == "act" else "", "", "", "") for l, (_, kind) in enumerate(layers)))


def test_route_without_the_keyword_is_what_it_was(built_lib, monkeypatch):
    """stack_route without `no_grad` (and with no_grad=False) returns the same route whatever EVAL_CHAIN says: the stored one
    in eval mode (finalize "running", every activation stored), the training one in training"""
    import rows_mlp
    assert rows_mlp.EVAL_CHAIN is True or rows_mlp.EVAL_CHAIN is False
    stacks = dict(MODEL, **NOT_TAKEN)
    monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", False)
    want = {(s, t): rows_mlp.stack_route(t, *stacks[s]) for s in stacks for t in (True, False)}
    for flag in (True, False):
        monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", flag)
        for s, (N, cin, layers) in stacks.items():
            for t in (True, False):
                assert rows_mlp.stack_route(t, N, cin, layers) == want[s, t], (s, t)
                assert rows_mlp.stack_route(t, N, cin, layers, no_grad=False) == want[s, t], (s, t)
            assert rows_mlp.stack_route(True, N, cin, layers, no_grad=True) == want[s, True], s       # training under no_grad
            ev = want[s, False]
            assert not ev.training and all(r.gemm != "chain" and r.feed in ("input", "stored") for r in ev.layers)
            assert all(r.finalize == ("running" if r.kind == "bn" else "") for r in ev.layers)
            assert want[s, True].training and all(r.gemm != "chain" for r in want[s, True].layers)


def test_eval_under_no_grad_takes_the_chain_and_the_switch_turns_it_off(built_lib, monkeypatch):
    import rows_mlp
    monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", True)
    for s, (N, cin, layers) in MODEL.items():
        for rows in (N, 1, 256):
            assert rows_mlp.stack_route(False, rows, cin, layers, no_grad=True) == _chain(layers), (s, rows)
    for why, (N, cin, layers) in NOT_TAKEN.items():
        assert rows_mlp.stack_route(False, N, cin, layers, no_grad=True) == rows_mlp.stack_route(False, N, cin, layers), why
    monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", False)
    for s, (N, cin, layers) in MODEL.items():
        assert rows_mlp.stack_route(False, N, cin, layers, no_grad=True) == rows_mlp.stack_route(False, N, cin, layers), s


def test_predicate_is_false_exactly_where_the_library_refuses(built_lib):
    """eval_chain_ok asks omnipq_rows_infer_lds_bytes: -1 <=> False, in both libraries; the bytes are the header's sum"""
    import rows_mlp
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        for s, (N, cin, layers) in MODEL.items():
            widths = tuple(R.round_up(c, 32) for c, _ in layers)
            n = _lds_bytes(lib, R.round_up(cin, 32), widths)
            assert 0 < n <= 160 * 1024 and n == R.lds_bytes(R.round_up(cin, 32), widths)[0], (s, n)
            assert rows_mlp.eval_chain_ok(cin, widths)
        for why, (kpad, widths) in REFUSED.items():
            assert _lds_bytes(lib, kpad, widths) == -1, why
            # the predicate takes the input's channels and widens them as the kernel does
            assert rows_mlp.eval_chain_ok(kpad, widths) == (kpad > 0 and _lds_bytes(lib, R.round_up(kpad, 32), widths) >= 0), why
            assert not rows_mlp.eval_chain_ok(kpad, widths) or why == "kpad % 32"
        for why, (kpad, widths) in TAKEN.items():
            assert _lds_bytes(lib, kpad, widths) == R.lds_bytes(kpad, widths)[0] > 0, why
            assert rows_mlp.eval_chain_ok(kpad, widths), why
        lib.omnipq_rows_infer_lds_bytes.restype = ctypes.c_longlong
        assert lib.omnipq_rows_infer_lds_bytes(32, 2, None) == -1
    lib = ctypes.CDLL(built_lib)
    # the 64-row tile where it fits, the 32-row one where only that does: the bytes are those of the tile the launch uses
    assert _lds_bytes(lib, 288, (288, 288, 128)) == 8 * 704 + 2 * 64 * (296 + 296)
    assert _lds_bytes(lib, 32, (288, 288)) == 8 * 576 + 2 * 64 * (296 + 296)
    assert _lds_bytes(lib, 1024, (512, 512)) == 8 * 1024 + 2 * 32 * (1032 + 520)
    assert _lds_bytes(lib, 32, (64,)) == 8 * 64 + 2 * 64 * (40 + 72)


def test_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """EINVAL for every refused shape, a NULL required pointer and an incomplete BatchNorm quadruple; the pointers are never
    dereferenced on the device and no GPU is needed.  The layer records are real host memory (the call reads them)."""
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    Rec = ext.rows_infer_layer_struct()
    p, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)

    def records(kpad, widths, **bad):
        recs = (Rec * max(len(widths), 1))()
        for l, C in enumerate(widths):
            K = kpad if l == 0 else widths[l - 1]
            recs[l].W, recs[l].ldw, recs[l].C, recs[l].bias = 0x1000, K, C, 0x1000
            recs[l].gamma = recs[l].beta = recs[l].running_mean = recs[l].running_var = 0x1000
            recs[l].eps = 1e-5
        for field, value in bad.items():
            setattr(recs[0], field, value)
        return recs

    def call(lib, kpad, widths, n=70, cin=None, ldx=None, recs=None, x=p, out=p, layers=True, f32=0):
        recs = records(kpad, widths) if recs is None else recs
        cin = kpad if cin is None else cin
        return lib.omnipq_rows_infer(n, cin, cin if ldx is None else ldx, x, f32, len(widths),
                                     ctypes.byref(recs) if layers else null, out, null)

    for lib in ext._LIBS.values():
        for why, (kpad, widths) in REFUSED.items():
            assert call(lib, kpad, widths) == EINVAL, why
        kpad, widths = 32, (64, 64, 64)
        for name in ("x", "out"):
            assert call(lib, kpad, widths, **{name: null}) == EINVAL, name
        assert call(lib, kpad, widths, layers=False) == EINVAL
        assert call(lib, kpad, widths, out=ctypes.c_void_p(0x1008)) == EINVAL              # rows leave in 16-byte pieces
        assert call(lib, kpad, widths, cin=0) == EINVAL
        assert call(lib, kpad, widths, cin=3, ldx=2) == EINVAL                            # a pitch below the row
        assert call(lib, kpad, widths, n=-1) == EINVAL
        assert call(lib, kpad, widths, recs=records(kpad, widths, W=0)) == EINVAL
        for field in ("gamma", "beta", "running_mean", "running_var"):                    # three of the four
            assert call(lib, kpad, widths, recs=records(kpad, widths, **{field: 0})) == EINVAL, field
        assert call(lib, kpad, widths, recs=records(kpad, widths, ldw=24)) == EINVAL      # a pitch below the contraction length
        assert call(lib, kpad, widths, recs=records(kpad, widths, ldw=36)) == EINVAL      # ... or no multiple of 8
        # no row: a no-op that succeeds, after the checks; so does a stack without BatchNorm and without bias
        assert call(lib, kpad, widths, n=0) == 0
        plain = records(kpad, widths, gamma=0, beta=0, running_mean=0, running_var=0, bias=0)
        assert call(lib, kpad, widths, n=0, recs=plain) == 0
        assert call(lib, 32, (64,), n=0, cin=3, ldx=6, f32=1) == 0
    with pytest.raises(TypeError, match="omnipq_rows_infer"):
        ext._lib.omnipq_rows_infer(70, 32, 32, p, 0, 3, p, p)                              # the stream is missing


def _recorded(name, eval_chain, switch):
    """the events of the golden table's `name`/eval case with run() called as the model's call sites call it"""
    import rows_mlp
    case = G._case([G.STACKS[name]], training=False, backward=False)
    real_run, saved = rows_mlp.run, rows_mlp.EVAL_CHAIN
    rows_mlp.run = lambda *a, **kw: real_run(*a, eval_chain=eval_chain, **kw)
    rows_mlp.EVAL_CHAIN = switch
    try:
        return G.run_case(case)
    finally:
        rows_mlp.run, rows_mlp.EVAL_CHAIN = real_run, saved


@pytest.mark.parametrize("name", ["pos", "vote", "head", "head_cat", "fp"])
def test_opted_in_eval_forward_is_one_chain_call(built_lib, name):
    """With the recorder of tests/golden/make_golden_rows_calls.py: the opted-in eval forward issues exactly ONE call besides
    the preparation of its weights -- omnipq_rows_infer -- where the stored route issues a GEMM per layer, omnipq_bnrelu per
    BatchNorm layer and omnipq_pad_rows_e16 in front of a narrow input.  (omnipq_prep_weight, f32 parameter -> e16 operand, is
    recorded once per layer on both routes: the recorder's parameters are fresh; inside a model's weight arena they are views
    of the step's one launch.)  With the switch off it issues exactly the recorded `/eval` sequence."""
    import rows_mlp
    with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "rows_mlp_calls.json")) as fh:
        golden = G.expand(json.load(fh))[name + "/eval"]
    cin, layers, n = G.STACKS[name][:3]
    before = rows_mlp.eval_chain_uses
    events = _recorded(name, True, True)
    assert rows_mlp.eval_chain_uses == before + 1
    preps = [e for e in golden if e[0] == "omnipq_prep_weight"]
    assert len(preps) == len(layers)
    assert [e for e in events if e[0] == "omnipq_prep_weight"] == preps
    rest = [e for e in events if e[0] != "omnipq_prep_weight"]
    f32 = int(len(G.STACKS[name]) > 3 and bool(G.STACKS[name][3].get("f32")))
    assert rest == [["omnipq_rows_infer", n, cin, cin, "p", f32, len(layers), "p", "p"]], events
    # switch off, or not opted in: the recorded sequence, nothing of the chain
    assert _recorded(name, True, False) == golden
    assert _recorded(name, False, True) == golden
    assert rows_mlp.eval_chain_uses == before + 1


def test_opted_in_pair_is_two_chain_calls_and_training_keeps_its_sequence(built_lib):
    import rows_mlp
    with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "rows_mlp_calls.json")) as fh:
        golden = G.expand(json.load(fh))
    real = rows_mlp.run_pair
    rows_mlp.run_pair = lambda *a, **kw: real(*a, eval_chain=True, **kw)
    try:
        before = rows_mlp.eval_chain_uses
        events = G.run_case(G._case([G.PAIR_A, G.PAIR_B], training=False, backward=False))
        assert [e[0] for e in events if e[0] != "omnipq_prep_weight"] == ["omnipq_rows_infer"] * 2
        assert rows_mlp.eval_chain_uses == before + 2
        # training through the opted-in call sites: the recorded sequence, forward and backward
        assert G.run_case(G._case([G.PAIR_A, G.PAIR_B])) == golden["pair/equal"]
        assert rows_mlp.eval_chain_uses == before + 2
    finally:
        rows_mlp.run_pair = real


def test_symbols_are_declared_exported_and_reported(built_lib):
    """the header's declarations, the libraries' signature text and the record line, in both element-type libraries"""
    import re
    want = {"omnipq_rows_infer": ("i", "lilpiippp"), "omnipq_rows_infer_lds_bytes": ("l", "iip"),
            "omnipq_rows_infer_layer_record": ("s", "")}
    declared = capi.declared_signatures()
    assert {n: declared[n] for n in want} == want
    assert not any(n in capi.plan_aware() for n in want)
    # this test's own reading of the record in include/omnipq_decoder.h
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(capi.INCLUDE, "omnipq_decoder.h")).read(), flags=re.S)
    body = re.search(r"struct\s+omnipq_rows_infer_layer\s*\{(.*?)\}\s*;", text, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        toks = stmt.replace("*", " * ").replace(",", " , ").split()
        if not toks:
            continue
        base = [t for t in toks if t in ("void", "int", "float")][0]
        names = " ".join(toks[toks.index(base) + 1:]).split(" , ")
        fields += [(n.replace("*", "").strip(), "p" if "*" in n else {"int": "i", "float": "f"}[base]) for n in names]
    assert fields == [("W", "p"), ("ldw", "i"), ("C", "i"), ("bias", "p"), ("gamma", "p"), ("beta", "p"), ("running_mean", "p"),
                      ("running_var", "p"), ("eps", "f"), ("relu", "i")]
    line = "struct omnipq_rows_infer_layer " + " ".join(f"{f}:{t}" for f, t in fields)
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        assert {n: got[n] for n in want} == want, path
        assert all(hasattr(lib, n) for n in want), path
        lib.omnipq_rows_infer_layer_record.restype = ctypes.c_char_p
        assert lib.omnipq_rows_infer_layer_record().decode() == line, path
        assert lib.omnipq_abi_version() == 5                      # an addition only
    import pointnet2_utils
    Rec = pointnet2_utils._load_ext().rows_infer_layer_struct()
    assert [f for f, _ in Rec._fields_] == [f for f, _ in fields] and ctypes.sizeof(Rec) == 64
    assert (Rec.ldw.offset, Rec.C.offset, Rec.bias.offset, Rec.gamma.offset, Rec.eps.offset, Rec.relu.offset) == (8, 12, 16, 24, 56, 60)
    assert torch.bfloat16 in pointnet2_utils._load_ext()._LIBS
