"""ctypes view of libomnipq_pointops.so for tests: raw device pointers + stream, nothing else."""
import ctypes
import os
import re

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(REPO, "omni-pq_amd", "lib", "libomnipq_pointops.so")
INCLUDE = os.path.join(REPO, "include")


def declared_symbols():
    """Every function the public headers (include/*.h) declare."""
    names = set()
    for fn in sorted(os.listdir(INCLUDE)):
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(INCLUDE, fn)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names.update(re.findall(r"\b(omnipq_\w+)\s*\(", text))
    return sorted(names)


def declared_signatures():
    """{name: (return letter, parameter letters)} of every function the public headers declare, in the letters of
    omnipq_entry_point_signatures() (include/omnipq_pointops.h).  The tests' OWN reading of the headers, statement by
    statement -- not the function omni-pq_amd/build.py compiles into the library."""
    scalars = {("int",): "i", ("unsigned",): "u", ("unsigned", "int"): "u", ("long", "long"): "l", ("float",): "f",
               ("double",): "d"}
    returns = {("int",): "i", ("long", "long"): "l", ("void",): "v", ("const", "char", "*"): "s"}
    out = {}
    for fn in sorted(os.listdir(INCLUDE)):
        if not fn.endswith(".h"):
            continue
        text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, fn)).read(), flags=re.S)
        text = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
        text = text.replace('extern "C" {', " ")
        text = re.sub(r"\{[^{}]*\}", " ", text)                    # struct bodies: their fields end in `;` too
        for stmt in text.split(";"):
            if "(" not in stmt:
                continue
            head, _, rest = stmt.partition("(")
            params = rest[:rest.rindex(")")]
            *ret, name = head.replace("*", " * ").split()
            assert name.startswith("omnipq_") and name not in out, (fn, stmt)
            letters = ""
            for prm in ([] if params.split() == ["void"] else params.split(",")):
                toks = prm.replace("*", " * ").split()
                if toks[:3] == ["const", "omnipq_row_plan", "*"]:
                    letters += "P"
                elif "*" in toks or "[" in prm:
                    letters += "p"
                else:
                    letters += scalars[tuple(toks[:-1])]          # KeyError: a type the signature letters do not cover
            out[name] = (returns[tuple(ret)], letters)
    return out


def reported_signatures(lib_handle):
    """{name: (return letter, parameter letters)} as the loaded library reports them; every line must be well-formed"""
    lib_handle.omnipq_entry_point_signatures.restype = ctypes.c_char_p
    out = {}
    for line in lib_handle.omnipq_entry_point_signatures().decode().splitlines():
        fields = line.split()
        assert len(fields) in (2, 3) and fields[0] not in out, line
        out[fields[0]] = (fields[1], fields[2] if len(fields) == 3 else "")
    return out


def declared_records():
    """({define: value}, {struct: [(field, letter, array length or None)]}) of the public headers, in the letters of
    omnipq_abi_records() (include/omnipq_pointops.h): every `#define OMNIPQ_*` that has a value, every `typedef struct`.  The
    tests' OWN reading, token by token -- not the function omni-pq_amd/build.py compiles into the library.  A value that is no
    integer or a field type outside the letters raises here."""
    scalars = {("int",): "i", ("unsigned",): "u", ("unsigned", "int"): "u", ("long", "long"): "l", ("float",): "f",
               ("double",): "d", ("unsigned", "long", "long"): "L"}
    texts = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, fn)).read(), flags=re.S)
             for fn in sorted(os.listdir(INCLUDE)) if fn.endswith(".h")]
    defines, structs = {}, {}
    for text in texts:
        for ln in text.splitlines():
            toks = ln.split()
            if len(toks) >= 3 and toks[0] == "#define" and toks[1].startswith("OMNIPQ_"):
                assert len(toks) == 3 and toks[1] not in defines, ln
                defines[toks[1]] = int(toks[2].rstrip("uU"))
    for text in texts:
        for chunk in text.split("typedef struct")[1:]:
            body, _, tail = chunk.partition("}")
            body = body.partition("{")[2]
            name = tail.partition(";")[0].strip()
            assert name.startswith("omnipq_") and "{" not in body and name not in structs, name
            fields = structs[name] = []
            for stmt in body.split(";"):
                for c in "*[],":
                    stmt = stmt.replace(c, f" {c} ")
                toks = stmt.split()
                if not toks:
                    continue
                n = 0
                while toks[n] in ("const", "unsigned", "int", "long", "float", "double", "void", "char"):
                    n += 1
                base = tuple(t for t in toks[:n] if t != "const")
                for decl in " ".join(toks[n:]).split(" , "):                 # `int a, b;` / `const float *x, *y;`
                    d = decl.split()
                    stars = d.count("*")
                    assert d[:stars] == ["*"] * stars and len(d) - stars in (1, 4), (name, stmt)
                    count = None
                    if len(d) - stars == 4:
                        assert d[stars + 1] == "[" and d[stars + 3] == "]", (name, stmt)
                        count = int(d[stars + 2]) if d[stars + 2].isdigit() else defines[d[stars + 2]]
                    fields.append((d[stars], "p" if stars else scalars[base], count))
    return defines, structs


def reported_records(lib_handle):
    """the same pair as the loaded library reports it (omnipq_abi_records); every line must be well-formed and sorted"""
    lib_handle.omnipq_abi_records.restype = ctypes.c_char_p
    lines = lib_handle.omnipq_abi_records().decode().splitlines()
    assert lines == sorted(lines)
    defines, structs = {}, {}
    for line in lines:
        kind, name, *rest = line.split()
        assert kind in ("define", "struct") and name not in defines and name not in structs, line
        if kind == "define":
            assert len(rest) == 1, line
            defines[name] = int(rest[0])
        else:
            fields = structs[name] = []
            for field in rest:
                m = re.fullmatch(r"(\w+):([iulLfdp])(?:\*(\d+))?", field)
                assert m, line
                fields.append((m.group(1), m.group(2), int(m.group(3)) if m.group(3) else None))
    return defines, structs


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.omnipq_error_string.restype = ctypes.c_char_p
    return _lib


def P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def lib_of(dtype):
    """(library built for the 16-bit element type `dtype`, every entry point typed from the signatures it reports; the
    binding module) -- (None, module) when this build has no library for that type (pointnet2/_ext.py: _LIBS)"""
    import sa_fused
    ext = sa_fused._ext
    return ext._LIBS.get(dtype), ext


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def plan_aware():
    """Entry points of include/omnipq_sa.h that take `const omnipq_row_plan *plan` (the argument before the stream)."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, "omnipq_sa.h")).read(), flags=re.S)
    return frozenset(m.group(1) for m in re.finditer(r"\b(omnipq_\w+)\s*\(([^;{}()]*)\)\s*;", text)
                     if "omnipq_row_plan *plan" in m.group(2))


PLAN_AWARE = plan_aware()


def call(name, *args, plan=None):
    """plan: a ctypes pointer to an omnipq_row_plan for the plan-aware entry points (None = every row)"""
    if name in PLAN_AWARE:
        args = args + (plan,)
    rc = getattr(lib(), name)(*args, stream())
    return rc


def ok(name, *args, plan=None):
    rc = call(name, *args, plan=plan)
    assert rc == 0, f"{name} -> {rc}: {lib().omnipq_error_string(rc).decode()}"


def fps(xyz, m, flags=None):
    b, n, _ = xyz.shape
    out = torch.full((b, m), -7, device=xyz.device, dtype=torch.int32)
    tmp = torch.full((b, n), 1e10, device=xyz.device, dtype=torch.float32)
    if flags is None:
        ok("omnipq_furthest_point_sampling", b, n, m, P(xyz), P(tmp), P(out))
    else:
        ok("omnipq_furthest_point_sampling_ex", b, n, m, P(xyz), P(tmp), P(out), ctypes.c_uint(flags))
    rc = lib().omnipq_fps_check(stream())
    assert rc == 0, lib().omnipq_error_string(rc).decode()
    return out, tmp


def ball_query(new_xyz, xyz, radius, nsample):
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.full((b, m, nsample), -7, device=xyz.device, dtype=torch.int32)   # NOT zero-filled
    ok("omnipq_ball_query", b, n, m, ctypes.c_float(radius), nsample, P(new_xyz), P(xyz), P(idx))
    return idx


def ball_query_grid(new_xyz, xyz, radius, nsample):
    """the hash-grid variant of omnipq_ball_query: must give the same indices"""
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.full((b, m, nsample), -7, device=xyz.device, dtype=torch.int32)   # NOT zero-filled
    lib().omnipq_ball_query_grid_workspace_bytes.restype = ctypes.c_longlong
    ws = torch.empty(max(int(lib().omnipq_ball_query_grid_workspace_bytes(b, n)), 16), device=xyz.device, dtype=torch.uint8)
    ok("omnipq_ball_query_grid", b, n, m, ctypes.c_float(radius), nsample, P(new_xyz), P(xyz), P(idx), P(ws))
    return idx


def group_points(points, idx):
    b, c, n = points.shape
    _, m, s = idx.shape
    out = torch.empty((b, c, m, s), device=points.device)
    ok("omnipq_group_points", b, c, n, m, s, P(points), P(idx), P(out))
    return out


def group_points_grad(grad_out, idx, n):
    b, c, m, s = grad_out.shape
    out = torch.zeros((b, c, n), device=grad_out.device)
    ok("omnipq_group_points_grad", b, c, n, m, s, P(grad_out), P(idx), P(out))
    return out


def gather_points(points, idx):
    b, c, n = points.shape
    m = idx.shape[1]
    out = torch.empty((b, c, m), device=points.device)
    ok("omnipq_gather_points", b, c, n, m, P(points), P(idx), P(out))
    return out


def gather_points_grad(grad_out, idx, n):
    b, c, m = grad_out.shape
    out = torch.zeros((b, c, n), device=grad_out.device)
    ok("omnipq_gather_points_grad", b, c, n, m, P(grad_out), P(idx), P(out))
    return out


def three_nn(unknown, known):
    b, n, _ = unknown.shape
    m = known.shape[1]
    d2 = torch.empty((b, n, 3), device=unknown.device)
    idx = torch.empty((b, n, 3), device=unknown.device, dtype=torch.int32)
    ok("omnipq_three_nn", b, n, m, P(unknown), P(known), P(d2), P(idx))
    return d2, idx


def three_interpolate(points, idx, weight):
    b, c, m = points.shape
    n = idx.shape[1]
    out = torch.empty((b, c, n), device=points.device)
    ok("omnipq_three_interpolate", b, c, m, n, P(points), P(idx), P(weight), P(out))
    return out


def three_interpolate_grad(grad_out, idx, weight, m):
    b, c, n = grad_out.shape
    out = torch.zeros((b, c, m), device=grad_out.device)
    ok("omnipq_three_interpolate_grad", b, c, n, m, P(grad_out), P(idx), P(weight), P(out))
    return out
