"""Records what the host side of csrc/gemm_tn_bf16.hip ANSWERS, without a device: the return code of every argument check of
the weight-gradient (TN) entry points -- omnipq_gemm_tn_e16, ..._colsum, ..._affine, ..._xyz_affine, omnipq_gemm_tn_dz and
omnipq_gemm_tn_grouped -- and the four size functions (the slab policy and the three workspace sizes) over a grid of shapes.

    python tests/golden/make_golden_gemm_tn_host.py LIBRARY [OUT.json]

LIBRARY is a libomnipq_pointops.so built from the commit whose answers are the reference (the table in this directory was
recorded from the commit BEFORE the host side got one cut of the position axis and one workspace layout per route);
tests/test_gemm_tn_host_codes.py replays the table against the library of the tree it runs in.  Run it on a machine WITHOUT a
GPU: no case may reach a launch -- every case is a mutation of a valid call that an argument check rejects, or an empty
problem -- and the generator asserts exactly that of the reference library, but a library that wrongly accepted a case would
launch a kernel on the never-dereferenced pointer 0x1000.

The records that cross the ABI (omnipq_tn_problem, omnipq_row_plan) are built from the layout the LIBRARY reports
(omnipq_abi_records), never from a copy written here.
"""
import ctypes
import json
import os
import sys

PTR = 0x1000                     # "some non-null pointer": never dereferenced
EINVAL = 10001

_CTYPE = {"i": ctypes.c_int, "u": ctypes.c_uint, "l": ctypes.c_longlong, "L": ctypes.c_ulonglong, "f": ctypes.c_float,
          "d": ctypes.c_double, "p": ctypes.c_void_p, "P": ctypes.c_void_p, "v": None, "s": ctypes.c_char_p}


def signatures(lib):
    """{name: (return letter, parameter letters)} as the library reports them (omnipq_entry_point_signatures)"""
    lib.omnipq_entry_point_signatures.restype = ctypes.c_char_p
    out = {}
    for line in lib.omnipq_entry_point_signatures().decode().splitlines():
        fields = line.split()
        out[fields[0]] = (fields[1], fields[2] if len(fields) == 3 else "")
    return out


def structs(lib):
    """{name: ctypes.Structure} of omnipq_tn_problem and omnipq_row_plan, from the library's own record lines"""
    lib.omnipq_abi_records.restype = ctypes.c_char_p
    out = {}
    for line in lib.omnipq_abi_records().decode().splitlines():
        kind, name, *fields = line.split()
        if kind == "struct" and name in ("omnipq_tn_problem", "omnipq_row_plan"):
            members = []
            for field in fields:
                fname, _, t = field.partition(":")
                letter, _, count = t.partition("*")
                members.append((fname, _CTYPE[letter] * int(count) if count else _CTYPE[letter]))
            out[name] = type(name, (ctypes.Structure,), {"_fields_": members})
    return out


def run_case(lib, sigs, recs, fn, args):
    """Calls `fn` with the table's argument list: numbers as they are, pointers as addresses (0 = NULL), a row plan as None or
    {"rows": .., "row_w": 0 / 1}, the problem list of the grouped entry points as a list of {field: value}."""
    ret, letters = sigs[fn]
    assert len(letters) == len(args), (fn, letters, args)
    f = getattr(lib, fn)
    f.restype = _CTYPE[ret]
    f.argtypes = [_CTYPE[c] for c in letters]
    keep, conv = [], []
    for c, v in zip(letters, args):
        if c == "P" and v is not None:
            plan = recs["omnipq_row_plan"](rows_dev=PTR, row_w=PTR if v["row_w"] else None, goff=PTR, rows=v["rows"], gs=8)
            keep.append(plan)
            conv.append(ctypes.cast(ctypes.pointer(plan), ctypes.c_void_p))
        elif c == "p" and isinstance(v, list):
            rec = recs["omnipq_tn_problem"]
            assert all(sorted(q) == sorted(n for n, _ in rec._fields_) for q in v)      # every field of the library's record
            probs = (rec * max(len(v), 1))(*[rec(**{k: (x or None) if k in _PROBLEM_POINTERS else x for k, x in q.items()})
                                             for q in v])
            keep.append(probs)
            conv.append(ctypes.cast(probs, ctypes.c_void_p))
        elif c in "pP":
            conv.append(ctypes.c_void_p(v) if v else None)
        else:
            conv.append(int(v))
    return int(f(*conv))


# ---- the calls ------------------------------------------------------------------------------------------------------
# Parameter lists as include/omnipq_sa.h declares them, with the values of a VALID call (which is never made: it would launch).
M, N, P = 256, 128, 5000         # (no size equals PTR: the pointer parameters are found by that value)
_PLAN_STREAM = [("plan", None), ("stream", 0)]
_TN = [("M", M), ("N", N), ("P", P), ("A", PTR), ("lda", M), ("B", PTR), ("ldb", N)]
DZ_P = 70 * 128
_PROBLEM_POINTERS = ("A", "B", "colsum", "out", "ba", "bb", "rows_dev")
PROBLEM = dict(A=PTR, B=PTR, colsum=PTR, out=PTR, M=M, N=N, P=P, lda=M, ldb=N, out_rows=250, out_cols=120, out_ld=120, flags=0,
               rot=0, ba=0, bb=0, rows_dev=0)
BASE = {
    "omnipq_gemm_tn_e16": _TN + [("C", PTR), ("workspace", PTR)] + _PLAN_STREAM,
    "omnipq_gemm_tn_e16_colsum": _TN + [("C", PTR), ("workspace", PTR), ("colsum", PTR)] + _PLAN_STREAM,
    "omnipq_gemm_tn_e16_affine": _TN + [("ba", PTR), ("bb", PTR), ("C", PTR), ("workspace", PTR), ("colsum", PTR)] + _PLAN_STREAM,
    # (ldx = 4: the pitch of X0 follows the ldx rules, not ldb % 8)
    "omnipq_gemm_tn_e16_xyz_affine": _TN[:5] + [("X0", PTR), ("ldx", 4), ("W0", PTR), ("ldw0", 4), ("ba", PTR), ("bb", PTR),
                                                ("C", PTR), ("workspace", PTR)] + _PLAN_STREAM,
    "omnipq_gemm_tn_dz": [("C3", 256), ("N", 128), ("P", DZ_P), ("Y2", PTR), ("ldb", 128), ("ba", PTR), ("bb", PTR), ("hot", PTR),
                          ("unit_src", PTR), ("nsample", 32), ("workspace", PTR), ("slabs_out", 0), ("cs_offset_out", 0),
                          ("plan", {"rows": DZ_P, "row_w": 1}), ("stream", 0)],
    "omnipq_gemm_tn_grouped": [("nprob", 1), ("probs", [PROBLEM]), ("workspace", PTR), ("stream", 0)],
}


def mutations(fn):
    """[(what, {parameter: value})]: each breaks one rule of a valid call (or two, or makes the problem empty)"""
    names = [n for n, _ in BASE[fn]]
    out = []

    def add(what, **kw):
        assert all(k in names for k in kw), (fn, kw)
        out.append((what, kw))

    pointers = [n for n, v in BASE[fn] if v == PTR]
    if fn == "omnipq_gemm_tn_grouped":
        def prob(what, **kw):
            assert all(k in PROBLEM for k in kw), kw
            add(what, probs=[dict(PROBLEM, **kw)])

        add("nprob < 0", nprob=-1)
        add("nprob < 0 without problems", nprob=-1, probs=0, workspace=0)
        add("probs NULL", probs=0)
        add("workspace NULL", workspace=0)
        add("nprob == 0", nprob=0)
        add("nprob == 0 with everything NULL", nprob=0, probs=0, workspace=0)
        for n in ("M", "N"):
            prob(f"{n} == 0", **{n: 0})
            prob(f"{n} < 0", **{n: -8})
            prob(f"{n} % 8", **{n: PROBLEM[n] + 4})
        prob("P < 0", P=-1)
        for n in ("A", "B", "out"):
            prob(f"{n} NULL", **{n: 0})
        prob("lda % 8", lda=M + 4)
        prob("ldb % 8", ldb=N + 4)
        prob("out_rows == 0", out_rows=0)
        prob("out_cols == 0", out_cols=0, out_ld=0)
        prob("out_rows < 0", out_rows=-1)
        prob("out_cols < 0", out_cols=-1)
        prob("out_rows > M", out_rows=M + 1)
        prob("out_cols > N", out_cols=N + 1, out_ld=N + 1)
        prob("out_ld < out_cols", out_ld=119)
        prob("ba without bb", ba=PTR)
        prob("bb without ba", bb=PTR)
        prob("rot < 0", rot=-1)
        prob("rot + split > N", rot=3 | (126 << 8))
        prob("rot > out_cols", rot=121)
        prob("A NULL and M % 8", A=0, M=M + 4)
        prob("out NULL on a problem without positions", P=0, out=0)
        add("the second problem broken", nprob=2, probs=[PROBLEM, dict(PROBLEM, ldb=N + 4)])
        add("a broken problem past nprob == 0", nprob=0, probs=[dict(PROBLEM, M=-8)])
        add("a broken problem and no workspace", probs=[dict(PROBLEM, M=-8)], workspace=0)
        return out
    if fn == "omnipq_gemm_tn_dz":
        for n in ("C3", "N", "P"):
            add(f"{n} == 0", **{n: 0})
            add(f"{n} < 0", **{n: -128})
        add("C3 % 128", C3=192)
        add("N % 128", N=64, ldb=64)
        add("ldb % 8", ldb=132)
        add("ldb < N", ldb=120)
        for n in pointers:
            if n not in ("ba", "bb"):
                add(f"{n} NULL", **{n: 0})
        add("ba without bb", bb=0)
        add("bb without ba", ba=0)
        add("nsample < 8", nsample=4)
        add("nsample == 0", nsample=0)
        add("nsample not a power of two", nsample=48)
        add("no plan", plan=None)
        add("a plan of another row count", plan={"rows": DZ_P + 128, "row_w": 1})
        add("a plan without row weights", plan={"rows": DZ_P, "row_w": 0})
        add("C3 % 128 and no plan", C3=192, plan=None)
        add("Y2 NULL and nsample < 8", Y2=0, nsample=4)
        add("no plan and no operands", plan=None, ba=0, bb=0)
        return out

    for n in ("M", "N", "P"):
        add(f"{n} < 0", **{n: -1})
    add("M == 0", M=0)
    add("N == 0", N=0)
    add("M == 0 and N == 0", M=0, N=0)
    add("M < 0 and N == 0", M=-1, N=0)
    add("M == 0 and P < 0", M=0, P=-1)
    add("M == 0 with every pointer NULL", M=0, **{n: 0 for n in pointers})
    add("M == 0 with the operands NULL", M=0, A=0, C=0, workspace=0)
    add("M == 0 with broken pitches", M=0, lda=M + 4, N=N + 4)
    for n in pointers:
        if not (n == "colsum" and fn == "omnipq_gemm_tn_e16_affine"):        # (may be NULL there)
            add(f"{n} NULL", **{n: 0})
    add("M % 8", M=M + 4, lda=M + 8)
    add("N % 8", N=N + 4, **({"ldb": N + 8} if "ldb" in names else {}))
    add("lda % 8", lda=M + 4)
    add("A NULL and M % 8", A=0, M=M + 4, lda=M + 8)
    if "ldb" in names:
        add("ldb % 8", ldb=N + 4)
    if fn == "omnipq_gemm_tn_e16_colsum":
        add("colsum NULL on an empty problem", M=0, colsum=0)
        add("colsum NULL and M < 0", M=-1, colsum=0)
    if "ba" in names:
        add("ba NULL on an empty problem", M=0, ba=0)
        add("bb NULL on an empty problem", N=0, bb=0)
        add("ba NULL and M < 0", M=-1, ba=0)
    if "ldx" in names:
        add("ldx % 4", ldx=6)
        add("ldw0 % 4", ldw0=6)
        add("ldx < 3", ldx=0)
        add("ldw0 < 3", ldw0=0)
        add("ldx < 0", ldx=-4)
        add("ldx % 4 on an empty problem", M=0, ldx=6)
        add("W0 NULL on an empty problem", N=0, W0=0)
    return out


def _empty(fn, vals):
    """the calls that answer OMNIPQ_OK without launching"""
    if fn == "omnipq_gemm_tn_grouped":
        return vals["nprob"] == 0
    return fn != "omnipq_gemm_tn_dz" and (vals["M"] == 0 or vals["N"] == 0)


def _problem_lists():
    """the lists of the grouped size function: 1, 6 and 48 problems with and without colsum, members without positions, the
    largest P on both sides of the workgroup-target switch (65536), and totals on both clamps of the steps per workgroup
    (16: the small lists; 1024: 48 problems of a million rows) as well as between them (48 problems of 65535 / 65536 rows)"""
    shapes = [(512, 256), (256, 128), (288, 64), (2048, 288), (136, 72)]
    for n in (1, 6, 48):
        for colsum in (0, PTR):
            for max_p in (4096, 65535, 65536, 1 << 20):
                members = [max_p, 0, 4096, max_p, 8192, 100]
                yield [dict(PROBLEM, M=m, N=k, lda=m, ldb=k, out_rows=m, out_cols=k, out_ld=k, colsum=colsum, P=members[i % len(members)])
                       for i in range(n) for m, k in [shapes[i % len(shapes)]]]


def size_grid():
    """[(function, [arguments])] of the four size functions"""
    positions = [0, 1, 31, 32, 191, 192, 193, 4096, 40000, 262144, 1048576]
    out = []
    for tiles in (1, 2, 12, 529):
        for p in positions:
            for k_step in (32, 64):
                out.append(("omnipq_gemm_tn_slabs", [tiles, p, k_step]))
    # 1, 2, 12 and 529 tiles of 128 x 128; then M / N that are no multiples of 128 (2, 6 and 3 tiles)
    for m, n in [(128, 128), (256, 128), (512, 384), (2944, 2944), (200, 72), (136, 264), (8, 288)]:
        for p in positions:
            out.append(("omnipq_gemm_tn_workspace_floats", [m, n, p]))
    for c3 in (128, 256, 512):
        for n in (128, 256):
            for p in (512, 8192, 16896, 17408, 131072, 1048576):
                out.append(("omnipq_gemm_tn_dz_workspace_floats", [c3, n, p]))
    for probs in _problem_lists():
        out.append(("omnipq_gemm_tn_grouped_workspace_floats", [len(probs), probs]))
    return out


def record(lib_path):
    lib = ctypes.CDLL(lib_path)
    sigs, recs = signatures(lib), structs(lib)
    calls = []
    for fn in BASE:
        for what, kw in mutations(fn):
            args = [kw.get(n, v) for n, v in BASE[fn]]
            rc = run_case(lib, sigs, recs, fn, args)
            assert rc != 0 or _empty(fn, dict(zip([n for n, _ in BASE[fn]], args))), (fn, what, "would have launched")
            assert rc in (0, EINVAL), (fn, what, rc)
            calls.append({"fn": fn, "what": what, "args": args, "rc": rc})
    sizes = [{"fn": fn, "args": args, "n": run_case(lib, sigs, recs, fn, args)} for fn, args in size_grid()]
    return {"abi_version": int(lib.omnipq_abi_version()), "calls": calls, "sizes": sizes}


if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tn_host.json")
    table = record(sys.argv[1])
    with open(out, "w") as fh:
        fh.write("{\n\"abi_version\": %d,\n\"calls\": [\n" % table["abi_version"])
        fh.write(",\n".join(json.dumps(c) for c in table["calls"]))
        fh.write("\n],\n\"sizes\": [\n")
        fh.write(",\n".join(json.dumps(c) for c in table["sizes"]))
        fh.write("\n]\n}\n")
    print(f"{out}: {len(table['calls'])} calls, {len(table['sizes'])} sizes")
