"""Records what the host side of csrc/gemm_bf16.hip ANSWERS, without a device: the return code of every argument check of
the sixteen omnipq_gemm_nt_e16* entry points and the three workspace-size functions over a grid of shapes.

    python tests/golden/make_golden_gemm_nt_host.py LIBRARY [OUT.json]

LIBRARY is a libomnipq_pointops.so built from the commit whose answers are the reference (the table in this directory was
recorded from the commit BEFORE the entry points were put behind one dispatcher); tests/test_gemm_nt_host_codes.py replays the
table against the library of the tree it runs in.  Run it on a machine WITHOUT a GPU: no case may reach a launch -- every
case is a mutation of a valid call that an argument check rejects, or an empty problem -- and the generator asserts exactly
that of the reference library (non-zero, or zero for M == 0 / N == 0), but a library that wrongly accepted a case would launch
a kernel on the never-dereferenced pointer 0x1000.
"""
import ctypes
import json
import os
import sys

PTR = 0x1000                     # "some non-null pointer": never dereferenced
EINVAL, ETOOLARGE = 10001, 10002


class RowPlan(ctypes.Structure):
    """include/omnipq_sa.h: omnipq_row_plan"""
    _fields_ = [("rows_dev", ctypes.c_void_p), ("row_w", ctypes.c_void_p), ("goff", ctypes.c_void_p),
                ("rows", ctypes.c_longlong), ("gs", ctypes.c_int), ("pool_gamma", ctypes.c_void_p)]


_CTYPE = {"i": ctypes.c_int, "u": ctypes.c_uint, "l": ctypes.c_longlong, "f": ctypes.c_float, "d": ctypes.c_double,
          "p": ctypes.c_void_p, "P": ctypes.c_void_p, "v": None, "s": ctypes.c_char_p}


def signatures(lib):
    """{name: (return letter, parameter letters)} as the library reports them (omnipq_entry_point_signatures)"""
    lib.omnipq_entry_point_signatures.restype = ctypes.c_char_p
    out = {}
    for line in lib.omnipq_entry_point_signatures().decode().splitlines():
        fields = line.split()
        out[fields[0]] = (fields[1], fields[2] if len(fields) == 3 else "")
    return out


def run_case(lib, sigs, fn, args):
    """Calls `fn` with the table's argument list: numbers as they are, pointers as addresses (0 = NULL), a row plan as None or
    {"rows": .., "row_w": 0 / 1}."""
    ret, letters = sigs[fn]
    assert len(letters) == len(args), (fn, letters, args)
    f = getattr(lib, fn)
    f.restype = _CTYPE[ret]
    f.argtypes = [_CTYPE[c] for c in letters]
    keep, conv = [], []
    for c, v in zip(letters, args):
        if c == "P" and v is not None:
            plan = RowPlan(PTR, PTR if v["row_w"] else None, PTR, v["rows"], 8, None)
            keep.append(plan)
            conv.append(ctypes.cast(ctypes.pointer(plan), ctypes.c_void_p))
        elif c in "pP":
            conv.append(ctypes.c_void_p(v) if v else None)
        elif c in "fd":
            conv.append(float(v))                       # ("nan" is spelled as a string)
        else:
            conv.append(int(v))
    return int(f(*conv))


# ---- the calls ------------------------------------------------------------------------------------------------------
# Parameter lists as include/omnipq_sa.h declares them, with the values of a VALID call (which is never made: it would
# launch).  BIG rows are 70 row tiles of 128 (the partial-sum path, more than 64), N = 128, K = 64.
BIG, N, K = 70 * 128, 128, 64
_PLAN_STREAM = [("plan", None), ("stream", 0)]
_NT = [("M", BIG), ("N", N), ("K", K), ("A", PTR), ("lda", K), ("B", PTR), ("ldb", K), ("C", PTR), ("ldc", N)]
_FIN = [("fin_sums", PTR), ("count", 1024.0), ("gamma", PTR), ("beta", PTR), ("eps", 1e-5), ("momentum", 0.1),
        ("running_mean", PTR), ("running_var", PTR)]
_FIN_OUT = [("a_out", PTR), ("b_out", PTR), ("mean_out", PTR), ("invstd_out", PTR)]
_POOL = [("s", 8), ("ymax", PTR), ("ymin", PTR), ("amax", PTR), ("amin", PTR)]
_BN = [("a", PTR), ("b", PTR), ("mean", PTR), ("invstd", PTR)]
_XYZ = [("X0", PTR), ("ldx", 4), ("W0", PTR), ("ldw0", 4)]
BASE = {
    "omnipq_gemm_nt_e16": _NT + _PLAN_STREAM,
    "omnipq_gemm_nt_e16_stats": _NT + [("bias", 0), ("sums", PTR), ("workspace", PTR)] + _PLAN_STREAM,
    "omnipq_gemm_nt_e16_stats_pool": _NT + [("bias", 0), ("sums", PTR), ("workspace", PTR)] + _POOL + _PLAN_STREAM,
    "omnipq_gemm_nt_e16_affine": _NT[:5] + [("a_in", PTR), ("b_in", PTR)] + _NT[5:] +
                                 [("bias", 0), ("sums", PTR), ("workspace", PTR)] + _PLAN_STREAM,
    "omnipq_gemm_nt_e16_bnaffine": _NT[:5] + _FIN + [("conv_bias", 0)] + _FIN_OUT + _NT[5:] +
                                   [("bias", 0), ("sums", PTR), ("workspace", PTR)] + _PLAN_STREAM,
    "omnipq_gemm_nt_e16_bnaffine_pool": _NT[:5] + _FIN + [("conv_bias", 0)] + _FIN_OUT + _NT[5:] +
                                        [("bias", 0), ("sums", PTR), ("workspace", PTR)] + _POOL + _PLAN_STREAM,
    "omnipq_gemm_nt_e16_bnbwd": _NT + [("Y", PTR)] + _BN + [("sums", PTR), ("workspace", PTR)] + _PLAN_STREAM,
    "omnipq_gemm_nt_e16_dz_bnbwd": [("M", BIG), ("N", 128), ("C3", 256), ("Y2", PTR), ("lda", 128), ("B1", PTR), ("ldb1", 160),
                                    ("B2", PTR), ("ldb2", 256), ("hot", PTR), ("unit_src", PTR), ("nsample", 32), ("C", PTR),
                                    ("ldc", 128)] + _BN + [("sums", PTR), ("workspace", PTR), ("X2out", PTR),
                                                           ("plan", {"rows": BIG, "row_w": 1}), ("stream", 0)],
    "omnipq_gemm_nt_e16_xyz_bnaffine": [("M", BIG), ("N", N), ("K", K)] + _XYZ + _FIN + _FIN_OUT +
                                       [("B", PTR), ("ldb", K), ("C", PTR), ("ldc", N), ("sums", PTR), ("workspace", PTR)] +
                                       _PLAN_STREAM,
    "omnipq_gemm_nt_e16_xyz_bnbwd": _NT[:7] + _XYZ + _BN + [("sums5", PTR), ("workspace", PTR)] + _PLAN_STREAM,
    "omnipq_gemm_nt_e16_bias": _NT + [("bias", PTR), ("stream", 0)],
    "omnipq_gemm_nt_e16_relu_dropout": _NT + [("bias", PTR), ("dropout_p", 0.5), ("seed_ptr", PTR), ("salt", 7), ("stream", 0)],
    "omnipq_gemm_nt_e16_mask": _NT + [("H", PTR), ("dropout_p", 0.5), ("stream", 0)],
    "omnipq_gemm_nt_e16_ws": _NT + [("bias", PTR), ("workspace", PTR), ("stream", 0)],
    "omnipq_gemm_nt_e16_f32": _NT + [("stream", 0)],
    "omnipq_gemm_nt_e16_splitk": _NT[:7] + [("C", PTR), ("slabs", 4), ("workspace", PTR), ("stream", 0)],
}
SMALL = 64 * 128                 # 64 row tiles: the statistics go straight to f64 atomics


def mutations(fn):
    """[(what, {parameter: value})]: each breaks one rule of a valid call (or makes the problem empty)"""
    names = [n for n, _ in BASE[fn]]
    base = dict(BASE[fn])
    out = []

    def add(what, **kw):
        assert all(k in names for k in kw), (fn, kw)
        out.append((what, kw))

    pointers = [n for n, v in BASE[fn] if v == PTR]
    if fn == "omnipq_gemm_nt_e16_dz_bnbwd":
        for n in ("M", "N", "C3"):
            add(f"{n} == 0", **{n: 0})
            add(f"{n} < 0", **{n: -128})
        for n in pointers:
            if n != "X2out":
                add(f"{n} NULL", **{n: 0})
        add("N % 128", N=64, lda=64, ldc=64, ldb1=96)
        add("C3 % 128", C3=192)
        add("lda, ldc % 8", lda=132, ldc=132)
        add("ldb1 % 8", ldb1=164)
        add("ldb2 % 8", ldb2=260)
        add("lda != ldc", ldc=136)
        add("lda < N", lda=120, ldc=120)
        add("ldb1 < N + 32", ldb1=152)
        add("ldb2 < C3", ldb2=248)
        add("N + 32 > kAffMaxK", N=1024, lda=1024, ldc=1024, ldb1=1056)
        add("nsample < 8", nsample=4)
        add("nsample not a power of two", nsample=48)
        add("no plan", plan=None)
        add("a plan of another row count", plan={"rows": BIG + 128, "row_w": 1})
        add("a plan without row weights", plan={"rows": BIG, "row_w": 0})
        add("64 row tiles", M=SMALL, plan={"rows": SMALL, "row_w": 1})
        return out

    mult = 4 if fn in ("omnipq_gemm_nt_e16_f32", "omnipq_gemm_nt_e16_splitk") else 8
    for n in ("M", "N", "K"):
        add(f"{n} < 0", **{n: -1})
    add("M == 0", M=0)
    add("N == 0", N=0)
    add("M < 0 and N == 0", M=-1, N=0)
    add("M == 0 with every pointer NULL", M=0, **{n: 0 for n in pointers})
    for n in pointers:
        # (these may be NULL: C of ..._bnaffine_pool is the no-store form, see below; ..._affine / ..._bnaffine without sums
        # are the forms without statistics; ..._ws without a workspace does not split)
        valid = n in ("running_mean", "running_var", "bias", "seed_ptr") or \
            (n, fn) in (("C", "omnipq_gemm_nt_e16_bnaffine_pool"), ("workspace", "omnipq_gemm_nt_e16_ws")) or \
            (n == "sums" and fn in ("omnipq_gemm_nt_e16_affine", "omnipq_gemm_nt_e16_bnaffine"))
        if not valid:
            add(f"{n} NULL", **{n: 0})
    add("K % 32", K=K + 1)
    if "ldc" in names:
        add(f"N % {mult}", N=N + mult // 2, ldc=N + mult)
        add(f"ldc % {mult}", ldc=N + mult + mult // 2)
    else:
        add(f"N % {mult}", N=N + mult // 2)
    for n in ("lda", "ldb"):
        if n in names:
            add(f"{n} % 8", **{n: K + 4})
    if "workspace" in names and "sums" in names:
        add("more than 64 row tiles without a workspace", workspace=0)
    if "s" in names:
        add("s == 0", s=0)
        add("s < 0", s=-8)
        add("s does not divide 128", s=3, M=BIG // 128 * 129)
        add("s does not divide M", M=BIG + 4)
        add("M == 0 with s == 0", M=0, s=0)
    if "fin_sums" in names:
        add("count == 0", count=0.0)
        add("count < 0", count=-1.0)
        add("count NaN", count="nan")
        add("running_mean without running_var", running_var=0)
        add("running_var without running_mean", running_mean=0)
        add("fin_sums NULL on an empty problem", M=0, fin_sums=0)
    if "ldx" in names:
        add("ldx % 4", ldx=6)
        add("ldw0 % 4", ldw0=6)
        add("ldx < 3", ldx=0)
        add("ldw0 < 3", ldw0=0)
        add("64 row tiles", M=SMALL)
    if fn in ("omnipq_gemm_nt_e16_affine", "omnipq_gemm_nt_e16_bnaffine", "omnipq_gemm_nt_e16_bnaffine_pool"):
        add("K > kAffMaxK", K=1056, lda=1056, ldb=1056)
    if fn == "omnipq_gemm_nt_e16_affine":
        add("a_in NULL on an empty problem", M=0, a_in=0)
        add("C NULL without sums", C=0, sums=0)
    if fn == "omnipq_gemm_nt_e16_bnaffine_pool":
        add("no store on 64 row tiles", M=SMALL, C=0)
        add("no store on 64 row tiles with a plan", M=SMALL, C=0, plan={"rows": SMALL, "row_w": 1})
        add("no store without a workspace", C=0, workspace=0)
        add("sums NULL on an empty problem", M=0, sums=0)
    if fn == "omnipq_gemm_nt_e16_xyz_bnaffine":
        add("K > kXgMaxC", K=288, ldb=288)
        add("64 row tiles with a plan", M=SMALL, plan={"rows": SMALL, "row_w": 1})
    if fn == "omnipq_gemm_nt_e16_xyz_bnbwd":
        add("N > kXgMaxC", N=264)
    if "dropout_p" in names:
        add("dropout_p < 0", dropout_p=-0.125)
        add("dropout_p == 1", dropout_p=1.0)
        add("dropout_p NaN", dropout_p="nan")
    if fn == "omnipq_gemm_nt_e16_relu_dropout":
        add("dropout without a seed", seed_ptr=0)
        add("M * ldc == 2^32", M=1 << 20, N=4096, ldc=4096)
        add("M * ldc == 2^32 and dropout_p == 1", M=1 << 20, N=4096, ldc=4096, dropout_p=1.0)
        add("M * ldc == 2^32 on K % 32", M=1 << 20, N=4096, ldc=4096, K=K + 1)
    if fn == "omnipq_gemm_nt_e16_f32":
        add("ldc < N", ldc=N - 4)
    if fn == "omnipq_gemm_nt_e16_splitk":
        add("slabs == 0", slabs=0)
        add("slabs == 0 on an empty problem", slabs=0, M=0)
    assert base
    return out


def size_grid():
    """[(function, [arguments])] of the three workspace-size functions"""
    rows = [0, 1, 127, 128, 4096, 64 * 128 - 1, 64 * 128, 64 * 128 + 1, 65 * 128, 65 * 128 + 1, 10240, 1 << 20]
    out = []
    for M in rows:
        for n in (8, 128, 256, 288):
            out.append(("omnipq_gemm_nt_stats_workspace_floats", [M, n]))
            out.append(("omnipq_gemm_nt_xyz_workspace_floats", [M, n]))
    shapes = [(4096, 288, 2048), (4096, 288, 864), (4096, 2048, 288), (4096, 864, 288), (2048, 288, 2048), (1024, 288, 2048),
              (512, 128, 4096), (8192, 288, 2048), (16384, 288, 2048), (16385, 288, 2048), (64 * 128, 256, 1024),
              (65 * 128, 256, 1024), (128, 128, 512), (4096, 32, 8192), (1 << 20, 128, 2048)]
    for M, n, _ in shapes:
        for k in (32, 256, 288, 736, 768, 1024, 2048):
            out.append(("omnipq_gemm_nt_workspace_floats", [M, n, k]))
    for M, n, k in shapes:
        out.append(("omnipq_gemm_nt_workspace_floats", [M, n, k]))
    return out


def record(lib_path):
    lib = ctypes.CDLL(lib_path)
    sigs = signatures(lib)
    calls = []
    for fn in BASE:
        for what, kw in mutations(fn):
            args = [kw.get(n, v) for n, v in BASE[fn]]
            rc = run_case(lib, sigs, fn, args)
            vals = dict(zip([n for n, _ in BASE[fn]], args))
            empty = vals["M"] == 0 or vals["N"] == 0
            assert rc != 0 or empty, (fn, what, "would have launched")
            assert rc in (0, EINVAL, ETOOLARGE), (fn, what, rc)
            calls.append({"fn": fn, "what": what, "args": args, "rc": rc})
    sizes = [{"fn": fn, "args": args, "floats": run_case(lib, sigs, fn, args)} for fn, args in size_grid()]
    return {"abi_version": int(lib.omnipq_abi_version()), "calls": calls, "sizes": sizes}


if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_nt_host.json")
    table = record(sys.argv[1])
    with open(out, "w") as fh:
        fh.write("{\n\"abi_version\": %d,\n\"calls\": [\n" % table["abi_version"])
        fh.write(",\n".join(json.dumps(c) for c in table["calls"]))
        fh.write("\n],\n\"sizes\": [\n")
        fh.write(",\n".join(json.dumps(c) for c in table["sizes"]))
        fh.write("\n]\n}\n")
    print(f"{out}: {len(table['calls'])} calls, {len(table['sizes'])} sizes")
