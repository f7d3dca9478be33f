"""CPU (needs the built libraries, no GPU): the host side of the inference stage kernel (csrc/sa_infer.hip) -- which route
sa_fused.stage_route gives an eval stage with and without `no_grad`, the predicate that asks the library for its limits, the
argument checks of omnipq_sa_infer that run before anything is launched, and the three new symbols' declarations."""
import ctypes

import pytest

import capi

EINVAL = 10001
# name: (N, M, S, cin_raw, widths, features): the five stages of the benchmark model (tests/test_host_logic.py)
MODEL = {"sa1": (40000, 2048, 64, 0, (128, 128, 256), False),
         "sa2": (2048, 1024, 32, 256, (256, 256, 512), True),
         "sa3": (1024, 512, 16, 512, (256, 256, 512), True),
         "sa4": (512, 256, 16, 512, (256, 256, 512), True),
         "vote": (1024, 256, 16, 288, (288, 288, 288), True)}
KPAD = {"sa1": 32, "sa2": 288, "sa3": 544, "sa4": 544, "vote": 320}
# (S, kpad, widths) the kernel does not take, one per rule of include/omnipq_sa.h
REFUSED = {"S = 24": (24, 32, (64, 64, 64)), "a width of 48": (16, 32, (64, 48, 64)), "four layers": (16, 32, (64, 64, 64, 64)),
           "a width of 672": (16, 32, (64, 672, 64)), "no layer": (16, 32, ()), "kpad % 32": (16, 48, (64, 64)),
           "more LDS than a CU has": (16, 1056, (640, 640, 640))}
TAKEN = {"one layer": (16, 32, (64,)), "two layers": (128, 32, (32, 64)), "the widest": (32, 32, (640, 320, 640))}


def _lds_bytes(lib, S, kpad, widths):
    lib.omnipq_sa_infer_lds_bytes.restype = ctypes.c_longlong
    arr = (ctypes.c_int * max(len(widths), 1))(*widths)
    return int(lib.omnipq_sa_infer_lds_bytes(S, kpad, len(widths), arr))


def _route(sa_fused, stage, training, B=8, **kw):
    N, M, S, cin_raw, widths, feats = MODEL[stage]
    return sa_fused.stage_route(training, B, N, M, S, cin_raw, widths, feats, False, False, **kw)


def test_route_without_the_keyword_is_what_it_was(built_lib, monkeypatch):
    """stage_route without `no_grad` (and with no_grad=False) returns, for the five model stages, the stored tuple in eval mode
    and the same training route whatever EVAL_CHAIN says"""
    import sa_fused
    stored = sa_fused.StageRoute(False, "grouped", 0, False, ("stored", "stored"), ("running",) * 3, "", "y", False)
    assert sa_fused.EVAL_CHAIN is True or sa_fused.EVAL_CHAIN is False
    train = {s: _route(sa_fused, s, True) for s in MODEL}
    for flag in (True, False):
        monkeypatch.setattr(sa_fused, "EVAL_CHAIN", flag)
        for s in MODEL:
            assert _route(sa_fused, s, False) == stored and _route(sa_fused, s, False, no_grad=False) == stored, s
            assert _route(sa_fused, s, True) == train[s] and _route(sa_fused, s, True, no_grad=True) == train[s], s
            assert train[s].training and train[s].first != "chain"


def test_eval_under_no_grad_takes_the_chain_and_the_switch_turns_it_off(built_lib, monkeypatch):
    import sa_fused
    monkeypatch.setattr(sa_fused, "EVAL_CHAIN", True)
    chain = sa_fused.StageRoute(False, "chain", 0, False, ("lds", "lds"), ("folded",) * 3, "", "y", False)
    for s in MODEL:
        for B in (1, 8):
            assert _route(sa_fused, s, False, B=B, no_grad=True) == chain, (s, B)
        # a plan that arrives with idx is ignored
        assert _route(sa_fused, s, False, no_grad=True, plan_gs=8, plan_unit_map=True) == chain, s
    # one and two layers
    r = sa_fused.stage_route(False, 1, 128, 4, 16, 16, (64,), True, False, False, no_grad=True)
    assert (r.first, r.feed, r.finalize) == ("chain", (), ("folded",))
    r = sa_fused.stage_route(False, 1, 256, 5, 128, 6, (32, 64), True, False, False, no_grad=True)      # 6 channels travel as 8
    assert (r.first, r.feed, r.finalize) == ("chain", ("lds",), ("folded", "folded"))
    # a shape the kernel does not take keeps the stored route
    stored4 = sa_fused.stage_route(False, 1, 128, 4, 16, 16, (64, 64, 64, 64), True, False, False, no_grad=True)
    assert stored4.first == "grouped" and stored4.feed == ("stored",) * 3
    assert sa_fused.stage_route(False, 1, 128, 4, 24, 16, (64,), True, False, False, no_grad=True).first == "grouped"
    monkeypatch.setattr(sa_fused, "EVAL_CHAIN", False)
    stored = sa_fused.StageRoute(False, "grouped", 0, False, ("stored", "stored"), ("running",) * 3, "", "y", False)
    assert all(_route(sa_fused, s, False, no_grad=True) == stored for s in MODEL)


def test_use_counter_counts_the_chain_only(built_lib):
    import sa_fused
    chain = sa_fused.StageRoute(False, "chain", 0, False, ("lds", "lds"), ("folded",) * 3, "", "y", False)
    stored = sa_fused.StageRoute(False, "grouped", 0, False, ("stored", "stored"), ("running",) * 3, "", "y", False)
    before = sa_fused.eval_chain_uses
    sa_fused._count_uses(stored)
    assert sa_fused.eval_chain_uses == before
    sa_fused._count_uses(chain)
    assert sa_fused.eval_chain_uses == before + 1
    sa_fused.eval_chain_uses = before


def test_predicate_is_false_exactly_where_the_library_refuses(built_lib):
    """eval_chain_ok asks omnipq_sa_infer_lds_bytes: -1 <=> False, in both libraries; the five model stages fit a CU"""
    import sa_fused
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        for s, (N, M, S, cin_raw, widths, _) in MODEL.items():
            n = _lds_bytes(lib, S, KPAD[s], widths)
            assert 0 < n <= 160 * 1024, (s, n)
            assert sa_fused.eval_chain_ok(S, KPAD[s], widths)
        for why, (S, kpad, widths) in REFUSED.items():
            assert _lds_bytes(lib, S, kpad, widths) == -1, why
            assert not sa_fused.eval_chain_ok(S, kpad, widths), why
        for why, (S, kpad, widths) in TAKEN.items():
            assert 0 < _lds_bytes(lib, S, kpad, widths) <= 160 * 1024, why
            assert sa_fused.eval_chain_ok(S, kpad, widths), why
        lib.omnipq_sa_infer_lds_bytes.restype = ctypes.c_longlong
        assert lib.omnipq_sa_infer_lds_bytes(16, 32, 2, None) == -1
    # what the header states: a | b of every layer, buffer A = rows x (max(kpad, C_1) + 8), buffer B = rows x (C_0 + 8)
    assert _lds_bytes(ctypes.CDLL(built_lib), 16, 544, (256, 256, 512)) == 8 * 1024 + 2 * 64 * (552 + 264)
    assert _lds_bytes(ctypes.CDLL(built_lib), 128, 32, (32, 64)) == 8 * 96 + 2 * 128 * (40 + 40)
    assert _lds_bytes(ctypes.CDLL(built_lib), 16, 32, (64,)) == 8 * 64 + 2 * 64 * 40


def test_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """EINVAL for every refused shape and for a NULL required pointer; the pointers are never dereferenced on the device and
    no GPU is needed.  The layer records are real host memory (the call reads them)."""
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    Rec = ext.sa_infer_layer_struct()
    p, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)

    def records(kpad, widths, **bad):
        recs = (Rec * max(len(widths), 1))()
        for l, C in enumerate(widths):
            K = kpad if l == 0 else widths[l - 1]
            recs[l].W, recs[l].ldw, recs[l].C = 0x1000, K, C
            recs[l].gamma = recs[l].beta = recs[l].running_mean = recs[l].running_var = 0x1000
            recs[l].eps = 1e-5
        for field, value in bad.items():
            setattr(recs[0], field, value)
        return recs

    def call(lib, S, kpad, widths, cin=0, recs=None, xyz=p, new_xyz=p, idx=p, feat=null, out_f32=p, out_pm=p, layers=True):
        recs = records(kpad, widths) if recs is None else recs
        return lib.omnipq_sa_infer(2, 64, 4, S, cin, kpad, 2.5, xyz, new_xyz, idx, feat, len(widths),
                                   ctypes.byref(recs) if layers else null, out_f32, out_pm, null)

    for lib in ext._LIBS.values():
        for why, (S, kpad, widths) in REFUSED.items():
            assert call(lib, S, kpad, widths) == EINVAL, why
        S, kpad, widths = 16, 32, (64, 64, 64)
        for name in ("xyz", "new_xyz", "idx", "out_f32", "out_pm"):
            assert call(lib, S, kpad, widths, **{name: null}) == EINVAL, name
        assert call(lib, S, kpad, widths, layers=False) == EINVAL
        assert call(lib, S, kpad, widths, cin=16, feat=null) == EINVAL                  # features without their pointer
        assert call(lib, S, kpad, widths, cin=12, feat=p) == EINVAL                     # cin % 8
        assert call(lib, S, kpad, widths, cin=32, feat=p) == EINVAL                     # kpad < cin + 3
        for field in ("W", "gamma", "beta", "running_mean", "running_var"):
            assert call(lib, S, kpad, widths, recs=records(kpad, widths, **{field: 0})) == EINVAL, field
        assert call(lib, S, kpad, widths, recs=records(kpad, widths, ldw=24)) == EINVAL   # a pitch below the contraction length
        assert call(lib, S, kpad, widths, recs=records(kpad, widths, ldw=36)) == EINVAL   # ... or no multiple of 8
        # no ball: a no-op that succeeds, after the checks
        recs = records(kpad, widths)
        assert lib.omnipq_sa_infer(0, 64, 4, S, 0, kpad, 2.5, p, p, p, null, 3, ctypes.byref(recs), p, p, null) == 0
    with pytest.raises(TypeError, match="omnipq_sa_infer"):
        ext._lib.omnipq_sa_infer(2, 64, 4, 16, 0, 32, 2.5, p, p, p, null, 3, p, p, p)      # the stream is missing


def test_symbols_are_declared_exported_and_reported(built_lib):
    """the header's declarations, the libraries' signature text and the record line, in both element-type libraries"""
    import os
    import re
    want = {"omnipq_sa_infer": ("i", "iiiiiifppppipppp"), "omnipq_sa_infer_lds_bytes": ("l", "iiip"),
            "omnipq_sa_infer_layer_record": ("s", "")}
    declared = capi.declared_signatures()
    assert {n: declared[n] for n in want} == want
    assert not any(n in capi.plan_aware() for n in want)
    # this test's own reading of the record in include/omnipq_sa.h
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(capi.INCLUDE, "omnipq_sa.h")).read(), flags=re.S)
    body = re.search(r"struct\s+omnipq_sa_infer_layer\s*\{(.*?)\}\s*;", text, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        toks = stmt.replace("*", " * ").replace(",", " , ").split()
        if not toks:
            continue
        base = [t for t in toks if t in ("void", "int", "float")][0]
        names = " ".join(toks[toks.index(base) + 1:]).split(" , ")
        fields += [(n.replace("*", "").strip(), "p" if "*" in n else {"int": "i", "float": "f"}[base]) for n in names]
    assert fields == [("W", "p"), ("ldw", "i"), ("C", "i"), ("gamma", "p"), ("beta", "p"), ("running_mean", "p"),
                      ("running_var", "p"), ("eps", "f")]
    line = "struct omnipq_sa_infer_layer " + " ".join(f"{f}:{t}" for f, t in fields)
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        assert {n: got[n] for n in want} == want, path
        assert all(hasattr(lib, n) for n in want), path
        lib.omnipq_sa_infer_layer_record.restype = ctypes.c_char_p
        assert lib.omnipq_sa_infer_layer_record().decode() == line, path
        assert lib.omnipq_abi_version() == 5                      # an addition only
    import pointnet2_utils
    Rec = pointnet2_utils._load_ext().sa_infer_layer_struct()
    assert [f for f, _ in Rec._fields_] == [f for f, _ in fields] and ctypes.sizeof(Rec) == 56
    assert (Rec.ldw.offset, Rec.C.offset, Rec.gamma.offset, Rec.eps.offset) == (8, 12, 16, 48)
