"""Builds the hand-written HIP library for gfx950 in-tree with hipcc -- twice, once per 16-bit element type:

    lib/libomnipq_pointops.so        e16 = bfloat16   (torch.autocast(bfloat16); also every index / f32 operator)
    lib/libomnipq_pointops_f16.so    e16 = IEEE half  (torch.autocast(float16); -DOMNIPQ_ELEM_F16, same sources, same entry points)

    python omni-pq_amd/build.py [--force]

No torch, no hipify, no cmake: one hipcc invocation per translation unit and element type, one link each.
hipcc cross-compiles gfx950 code objects on a machine without a GPU.
"""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libomnipq_pointops.so")
LIB_F16 = os.path.join(LIBDIR, "libomnipq_pointops_f16.so")
OBJDIR = os.path.join(HERE, "build")
# (library, object sub-directory, extra defines)
VARIANTS = [(LIB, "bf16", []), (LIB_F16, "f16", ["-DOMNIPQ_ELEM_F16=1"])]

# -ffp-contract=off: the index-producing kernels spell out every fma themselves (numerics
# contract in include/omnipq_pointops.h); nothing else may fuse.
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
          "-munsafe-fp-atomics", "-Wall", "-Wno-unused-function",
          "-I", os.path.join(REPO, "include"), "-I", CSRC]

# per-file extra flags.  fps.hip: the SLP vectorizer packs the per-point f32 arithmetic into
# v_pk_* pairs, which doubles the live registers of the 8-points-per-thread variants (134 spilled
# VGPRs); scalar code needs 79 and runs the same instruction count.
# attention.hip: -amdgpu-mfma-vgpr-form keeps the MFMA accumulators in the architectural registers.  The compiler's default
# put the output accumulators (which the online-softmax rescale also touches with VALU instructions) into AGPRs and copied them
# out and back around the matrix instructions of EVERY key block: 64 v_accvgpr_read / _write + 26 v_mov of the ~570 VALU
# instructions of a forward iteration.  With the flag: no copies, 160 / 184 / 204 registers instead of 192 / 212 / 236
# (forward: three waves per SIMD instead of two).
# eval_iou.hip: restates eval_det.box3d_iou in f64 product by product; a fused multiply-add would change an `inside`
# decision of the clipping.  COMMON says so already: the file's own entry keeps that true should COMMON ever change.
# detect.hip: the decoded heading is a product and a sum in f64, each rounded on its own, and its corners must keep the bits
# of eval_ops.hip's (csrc/box_geom.h); the same reason for an entry of its own.
# point_normals.hip: the neighbour order is decided by the f32 d2 of the numerics contract (its one fused step is spelled
# out, csrc/common.h: sumsq3) and the sign decisions of the smoothing and orientation by f64 sums stated term by term
# (include/omnipq_normals.h); the same reason again.
# layout_f1.hip: a corner distance is three f64 products and two sums as numpy forms them, compared with a threshold; the same
# reason once more.
EXTRA = {"fps.hip": ["-fno-slp-vectorize"], "attention.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
         "eval_iou.hip": ["-ffp-contract=off"], "detect.hip": ["-ffp-contract=off"],
         "point_normals.hip": ["-ffp-contract=off"], "layout_f1.hip": ["-ffp-contract=off"]}


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def sources_digest():
    """sha1 over the kernel sources (csrc/*.hip, csrc/*.h, include/*.h): stamped into the counter summaries under profiles/
    by tools/pmc_*.py and compared by bench.py, which labels a committed counter figure `stale` when the kernels have changed
    since it was taken."""
    import hashlib
    h = hashlib.sha1()
    inc = os.path.join(os.path.dirname(HERE), "include")
    files = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))]
    files += [os.path.join(inc, f) for f in sorted(os.listdir(inc)) if f.endswith(".h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


_SCALARS = {"int": "i", "unsigned": "u", "long long": "l", "float": "f", "double": "d"}
_RETURNS = {"int": "i", "long long": "l", "void": "v", "const char *": "s"}


def entry_point_signatures():
    """Every declaration of include/*.h as one line `name <ret> <params>`, one letter per type: i int, u unsigned, l long long,
    f float, d double, p any pointer (arrays and struct pointers included), P `const omnipq_row_plan *`; returns i, l, v void,
    s const char *.  Evaluated at BUILD time and compiled into the library (csrc/capi.hip: omnipq_entry_point_signatures), so
    that a binding asks the library it actually loaded how its entry points are called instead of parsing a header that may
    belong to another build.  A type that is not in this list fails the build: it is never guessed."""
    import re

    def words(s):
        return " ".join(s.replace("*", " * ").split())

    lines = []
    inc = os.path.join(REPO, "include")
    for header in sorted(f for f in os.listdir(inc) if f.endswith(".h")):
        with open(os.path.join(inc, header)) as fh:
            text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
        text = re.sub(r"^[ \t]*#.*$", ";", text, flags=re.M)
        for m in re.finditer(r"([^;{}()]*?)\b(omnipq_\w+)\s*\(([^;{}()]*)\)\s*;", text):
            name = m.group(2)
            ret = _RETURNS.get(words(m.group(1)))
            if ret is None:
                raise RuntimeError(f"{header}: {name}: return type `{words(m.group(1))}` has no signature letter")
            letters = ""
            params = [words(q) for q in m.group(3).split(",")]
            for q in ([] if params == ["void"] else params):
                decl = re.sub(r"\s*\w+\s*(\[[^\]]*\]\s*)*$", "", q)       # the type without the parameter's name / [n]
                if decl == "const omnipq_row_plan *":
                    letters += "P"
                elif "*" in q or "[" in q:
                    letters += "p"
                elif decl in _SCALARS:
                    letters += _SCALARS[decl]
                else:
                    raise RuntimeError(f"{header}: {name}: parameter `{q}` has no signature letter")
            lines.append(f"{name} {ret} {letters}".rstrip())
    return "".join(line + "\n" for line in sorted(lines))


_FIELDS = dict(_SCALARS, **{"unsigned long long": "L"})
_FIELD_CTYPES = {"i": ctypes.c_int, "u": ctypes.c_uint, "l": ctypes.c_longlong, "L": ctypes.c_ulonglong, "f": ctypes.c_float,
                 "d": ctypes.c_double, "p": ctypes.c_void_p}


def _parse_declarator(text):
    """`x`, `*x`, `y[N]` -> (field, is_pointer, dimension or None); None for anything else (`z[2][2]`, `(*f)(int)`)"""
    import re
    m = re.fullmatch(r"\s*((?:\*\s*)*)(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", text)
    return m and (m.group(2), bool(m.group(1)), m.group(3))


def _struct_fields(body, defines):
    """`field:t` / `field:t*n` per field of a struct body without comments.  ValueError(field): its type has no letter."""
    import re
    for stmt in body.split(";"):
        if not stmt.strip():
            continue
        # `const float *x, *y[N]`: the type stands once in front, every name carries its own `*` and `[n]`
        head = re.match(r"(.*?)((?:\*\s*)*\w+\s*(?:\[.*\])?)$", stmt.split(",")[0].strip())
        if not head:
            raise ValueError(stmt.strip())
        base = _FIELDS.get(" ".join(w for w in head.group(1).split() if w != "const"))
        for text in [head.group(2)] + stmt.split(",")[1:]:
            parsed = _parse_declarator(text)
            if parsed is None:
                raise ValueError(text.strip())
            field, is_pointer, dim = parsed
            letter = "p" if is_pointer else base
            count = None if dim is None else int(dim) if dim.isdigit() else defines.get(dim)
            if letter is None or (dim is not None and count is None):
                raise ValueError(field)
            yield f"{field}:{letter}" if dim is None else f"{field}:{letter}*{count}"


def abi_records():
    """What crosses the C ABI besides the calls, as sorted text: `define NAME value` per `#define OMNIPQ_* <decimal integer>` of
    include/*.h (a `u` / `l` suffix dropped; include guards have no value and are not listed) and
    `struct name field:t field:t*n ...` per `typedef struct {...} omnipq_*;`, fields in the header's order.  t is a letter of
    entry_point_signatures() or L unsigned long long; every pointer is p; *n is an array length, a define already resolved.
    Compiled into the library like the signatures (csrc/capi.hip: omnipq_abi_records) so that a binding builds its
    ctypes.Structure classes from the library it loaded.  A field whose type is not in this list fails the build."""
    import re
    texts = []
    inc = os.path.join(REPO, "include")
    for header in sorted(f for f in os.listdir(inc) if f.endswith(".h")):
        with open(os.path.join(inc, header)) as fh:
            texts.append((header, re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)))
    defines = {}
    for header, text in texts:
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(OMNIPQ_\w+)[ \t]+(-?\d+)[uUlL]*[ \t]*$", text, flags=re.M):
            defines[m.group(1)] = int(m.group(2))
    lines = [f"define {name} {value}" for name, value in defines.items()]
    for header, text in texts:
        for typedef in re.finditer(r"\btypedef\s+struct\b\s*\w*\s*\{(.*?)\}\s*(omnipq_\w+)\s*;", text, flags=re.S):
            body, struct = typedef.groups()
            try:
                nested = re.search(r"\{[^{}]*\}\s*(\w*)", body)
                if nested:
                    raise ValueError(nested.group(1))
                lines.append(" ".join([f"struct {struct}"] + list(_struct_fields(body, defines))))
            except ValueError as bad:
                raise RuntimeError(f"{header}: {struct}: field `{bad}` has no record letter") from None
    return "".join(line + "\n" for line in sorted(lines))


def record_struct(line):
    """`struct name field:t[*n] ...` -> the ctypes.Structure of that record.  The build's copy of what a binding does with the
    text (pointnet2/_ext.py: struct(), which cannot be imported here: it loads the library this build is about to make);
    tests/test_capi_symbols.py holds the two to the same fields."""
    _, name, *fields = line.split()
    members = []
    for field in fields:
        fname, _, kind = field.partition(":")
        letter, _, count = kind.partition("*")
        members.append((fname, _FIELD_CTYPES[letter] * int(count) if count else _FIELD_CTYPES[letter]))
    return type(name, (ctypes.Structure,), {"_fields_": members})


def layout_checks(records):
    """One static_assert per struct size and field offset of `records` (abi_records() text), the numbers taken from the
    ctypes.Structure a binding builds from that text: compiled into csrc/capi.hip next to the C definitions, so a layout Python
    would get wrong stops the build."""
    out = []
    for line in records.splitlines():
        if line.startswith("struct "):
            cls = record_struct(line)
            out.append(f'static_assert(sizeof({cls.__name__}) == {ctypes.sizeof(cls)}, "{cls.__name__}: size");')
            out += [f'static_assert(offsetof({cls.__name__}, {f}) == {getattr(cls, f).offset}, "{cls.__name__}.{f}: offset");'
                    for f, _ in cls._fields_]
    return "".join(s + "\n" for s in out)


# plain (not typedef'd) structs whose record line and layout checks are generated as well: each reports its own line through
# an entry point of its own (include/omnipq_optim.h: omnipq_lr_schedule_record) instead of through omnipq_abi_records()
PLAIN_STRUCTS = ("omnipq_lr_schedule",)


def plain_struct_record(name):
    """`struct name field:t[*n] ...` of the headers' plain `struct name {...};`, in the letters of abi_records()."""
    import re
    inc = os.path.join(REPO, "include")
    for header in sorted(f for f in os.listdir(inc) if f.endswith(".h")):
        with open(os.path.join(inc, header)) as fh:
            text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
        m = re.search(r"(?<!typedef)\s\bstruct\s+" + name + r"\s*\{([^{}]*)\}\s*;", text)
        if m:
            try:
                return " ".join([f"struct {name}"] + list(_struct_fields(m.group(1), {})))
            except ValueError as bad:
                raise RuntimeError(f"{header}: {name}: field `{bad}` has no record letter") from None
    raise RuntimeError(f"include/*.h define no `struct {name} {{...}};`")


def plain_struct_text():
    """Per struct of PLAIN_STRUCTS: its record line as the C string `<name>_record_text` and the static_asserts of
    layout_checks() for it, for the translation unit that owns the struct's *_record() entry point."""
    out = []
    for name in PLAIN_STRUCTS:
        line = plain_struct_record(name)
        out.append(f'static const char {name}_record_text[] = "{line}";\n' + layout_checks(line + "\n"))
    return "".join(out)


GENERATED = ("entry_points.inc", "abi_records.inc", "abi_layout_checks.inc", "plain_struct_records.inc")


def _c_string(text):
    return "".join(f'"{line}\\n"\n' for line in text.splitlines())


def _write_generated():
    """build/generated/: the two texts above as C string literals, the layout checks and the plain structs' records, each
    rewritten only when its content changes."""
    gen = os.path.join(OBJDIR, "generated")
    os.makedirs(gen, exist_ok=True)
    records = abi_records()
    for name, text in zip(GENERATED, (_c_string(entry_point_signatures()), _c_string(records), layout_checks(records),
                                     plain_struct_text())):
        path = os.path.join(gen, name)
        if not os.path.exists(path) or open(path).read() != text:
            with open(path, "w") as fh:
                fh.write(text)
    return gen


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """-> path of the bf16 library (the f16 twin is built next to it: LIB_F16)."""
    os.makedirs(LIBDIR, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    inc = os.path.join(REPO, "include")
    headers += [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")]
    gen = _write_generated()
    headers += [os.path.join(gen, f) for f in GENERATED]
    procs, links = [], []
    for lib, sub, defines in VARIANTS:
        objdir = os.path.join(OBJDIR, sub)
        os.makedirs(objdir, exist_ok=True)
        objs = []
        compiled = False
        for src in sources():
            obj = os.path.join(objdir, src[:-4] + ".o")
            objs.append(obj)
            if force or _stale(obj, [os.path.join(CSRC, src)] + headers):
                cmd = [hipcc()] + COMMON + ["-I", gen] + defines + EXTRA.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
                if verbose:
                    print(" ".join(cmd))
                procs.append((src, subprocess.Popen(cmd)))
                compiled = True
        links.append((lib, objs, compiled))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    for lib, objs, compiled in links:
        if force or compiled or _stale(lib, objs):
            cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
