"""CPU: the C-ABI library builds (hipcc cross-compiles gfx950 without a GPU), loads, and exports
every function include/omnipq_pointops.h declares.  No kernel is launched here."""
import ctypes
import capi


def both(built_lib):
    """the bfloat16 library and its IEEE-half twin (same sources, -DOMNIPQ_ELEM_F16: omni-pq_amd/build.py)"""
    return [built_lib, built_lib[:-3] + "_f16.so"]


def test_libraries_export_every_declared_symbol(built_lib):
    syms = capi.declared_symbols()
    assert len(syms) >= 25 and "omnipq_furthest_point_sampling" in syms and "omnipq_sa_gather" in syms
    assert "omnipq_gemm_nt_e16_stats" in syms
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        missing = [s for s in syms if not hasattr(lib, s)]
        assert not missing, (path, missing)


def test_libraries_have_gfx950_code_objects_with_their_mfma_opcode(built_lib, tmp_path):
    """Both libraries carry gfx950 code objects, and each one's matrix instructions are those of ITS element type only
    (disassembly of the bundled code objects: llvm-objdump --offloading extracts them next to its input)."""
    import glob
    import os
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    for path, opcode, other in zip(both(built_lib), ("v_mfma_f32_32x32x16_bf16", "v_mfma_f32_32x32x16_f16"),
                                   ("v_mfma_f32_32x32x16_f16", "v_mfma_f32_32x32x16_bf16")):
        blob = open(path, "rb").read()
        assert b"amdgcn-amd-amdhsa--gfx950" in blob
        if not os.path.exists(objdump):
            continue
        work = tmp_path / os.path.basename(path)
        work.mkdir()
        shutil.copy(path, work)
        subprocess.run([objdump, "--offloading", os.path.basename(path)], cwd=work, capture_output=True)
        asm = "".join(subprocess.run([objdump, "-d", f], capture_output=True, text=True).stdout
                      for f in glob.glob(str(work / "*gfx950")))
        if "v_mfma" not in asm:
            continue                                  # this objdump could not open the bundles: nothing to check
        assert asm.count(opcode) >= 100 and other not in asm, (path, asm.count(opcode), asm.count(other))


# gemm_nt_kernel<OUT_F32, STATS, AFF, T, XG, KRES, PLAN, DZ> and gemm_nt_pair_kernel<STATS, AFF> as the entry points of
# csrc/gemm_bf16.hip reach them (the list of the build before they were put behind one dispatcher).  Every instantiation
# costs about a second of compile time per element type: one that nothing can reach must not appear silently.
_F, _T = "false", "true"
_NT_KERNELS = {(_T, 0, _F, 64, 0, _F, _F, _F), (_T, 0, _F, 128, 0, _F, _F, _F)}                 # f32 out (and split-K)
_NT_KERNELS |= {(_F, st, aff, 64, 0, kres, _F, _F)                                              # 64 x 64 tiles
                for st, aff in ((0, _F), (1, _F), (0, _T), (1, _T), (3, _F), (5, _F)) for kres in (_T, _F)}
_NT_KERNELS |= {(_F, st, aff, 128, 0, _F, _F, _F)                                               # 128 x 128 tiles, every row
                for st, aff in ((0, _F), (1, _F), (2, _F), (0, _T), (1, _T), (2, _T), (3, _F), (4, _F), (5, _F))}
_NT_KERNELS |= {(_F, st, aff, 128, 0, _F, _T, _F) for st, aff in ((0, _F), (2, _F), (2, _T), (4, _F))}     # ... on a row plan
_NT_KERNELS |= {(_F, 4, _T, 128, 0, _F, _T, _T)}                                                # DZ: with a plan only
_NT_KERNELS |= {(_F, 2, _T, 128, 1, _F, plan, _F) for plan in (_T, _F)}                         # XG = 1
_NT_KERNELS |= {(_F, 4, _F, 128, 2, _F, plan, _F) for plan in (_T, _F)}                         # XG = 2
_NT_PAIR_KERNELS = {(0, _F), (1, _F), (0, _T), (1, _T), (3, _F), (5, _F)}


def test_nt_gemm_instantiations_are_the_listed_ones(built_lib, tmp_path):
    """The bf16 library holds exactly the 32 gemm_nt_kernel and 6 gemm_nt_pair_kernel instantiations written out above
    (demangled symbol tables of the bundled code objects)."""
    import glob
    import os
    import re
    import shutil
    import subprocess
    assert len(_NT_KERNELS) == 32 and len(_NT_PAIR_KERNELS) == 6
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        return
    shutil.copy(built_lib, tmp_path)
    subprocess.run([objdump, "--offloading", os.path.basename(built_lib)], cwd=tmp_path, capture_output=True)
    syms = "".join(subprocess.run([objdump, "-t", "-C", f], capture_output=True, text=True).stdout
                   for f in glob.glob(str(tmp_path / "*gfx950")))
    if "omnipq::" not in syms:
        return                                        # this objdump could not open the bundles: nothing to check

    def word(w):
        return w if w in (_F, _T) else int(w)

    found = {(m.group(1), tuple(word(w.strip()) for w in m.group(2).split(",")))
             for m in re.finditer(r"omnipq::(gemm_nt_kernel|gemm_nt_pair_kernel)<([^<>]*)>", syms)}
    want = {("gemm_nt_kernel", t) for t in _NT_KERNELS} | {("gemm_nt_pair_kernel", t) for t in _NT_PAIR_KERNELS}
    assert sorted(found - want) == [] and sorted(want - found) == [], (sorted(found - want), sorted(want - found))


def test_library_names_its_plan_aware_entry_points(built_lib):
    """the binding takes the set of plan-aware entry points from the LIBRARY it loaded (a build-time constant: the
    names whose reported signature has a `P`), and refuses a library of another ABI version; here: that set equals what the
    header of this tree declares, in both element-type libraries, and the binding's set is the library's."""
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        names = frozenset(n for n, (_, params) in capi.reported_signatures(lib).items() if "P" in params)
        assert names == capi.plan_aware() and len(names) >= 20, sorted(names ^ capi.plan_aware())
        assert all(hasattr(lib, n) for n in names)
    import pointnet2_utils
    assert pointnet2_utils._ext.PLAN_AWARE == capi.plan_aware()
    assert pointnet2_utils._ext.ABI_VERSION == lib.omnipq_abi_version() == 5


_CTYPE = {"i": ctypes.c_int, "u": ctypes.c_uint, "l": ctypes.c_longlong, "f": ctypes.c_float, "d": ctypes.c_double,
          "p": ctypes.c_void_p, "P": ctypes.c_void_p, "v": None, "s": ctypes.c_char_p}


def test_library_reports_the_signatures_its_headers_declare(built_lib):
    """Every function include/*.h declares is reported by both libraries with the header's return type, parameter count and
    letter per parameter (the headers read by tests/capi.py, not by the build), nothing else is reported, and the functions
    the binding loaded carry exactly these `restype` / `argtypes`."""
    want = capi.declared_signatures()
    assert sorted(want) == capi.declared_symbols() and len(want) >= 158
    assert want["omnipq_furthest_point_sampling_resume"] == ("i", "iiiiipppup")
    assert want["omnipq_copy_probe"] == ("i", "pplp") and want["omnipq_pair_hold"] == ("v", "")
    assert want["omnipq_error_string"] == ("s", "i") and want["omnipq_gemm_nt_workspace_floats"] == ("l", "iii")
    for path in both(built_lib):
        got = capi.reported_signatures(ctypes.CDLL(path))
        assert sorted(set(got) ^ set(want)) == [], path
        assert {n: got[n] for n in want if got[n] != want[n]} == {}, path
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    assert len(ext._LIBS) == 2
    for lib in ext._LIBS.values():
        for name, (ret, params) in want.items():
            fn = getattr(lib, name)
            assert fn.restype is _CTYPE[ret] and list(fn.argtypes) == [_CTYPE[c] for c in params], name


def test_build_refuses_a_type_without_a_signature_letter(built_lib, tmp_path, monkeypatch):
    """omni-pq_amd/build.py writes the reported text from the headers; a parameter or return type outside its list fails the
    build with the declaration's name instead of being guessed."""
    import pytest
    import build as omnipq_build
    inc = tmp_path / "include"
    inc.mkdir()
    monkeypatch.setattr(omnipq_build, "REPO", str(tmp_path))
    (inc / "a.h").write_text("/* x */\n#define N 3\nint omnipq_ok(int a, const float *b, long long v[N], unsigned f, void *stream);\n"
                             "void omnipq_none(void);\n")
    assert omnipq_build.entry_point_signatures() == "omnipq_none v\nomnipq_ok i ippup\n"
    (inc / "b.h").write_text("int omnipq_bad(int a, short b, void *stream);\n")
    with pytest.raises(RuntimeError, match="omnipq_bad"):
        omnipq_build.entry_point_signatures()
    (inc / "b.h").write_text("short omnipq_worse(int a);\n")
    with pytest.raises(RuntimeError, match="omnipq_worse"):
        omnipq_build.entry_point_signatures()


def test_build_refuses_a_struct_field_without_a_record_letter(built_lib, tmp_path, monkeypatch):
    """... and the same for what omni-pq_amd/build.py reports of structs and defines: the listed field types, several names per
    declaration, an array dimensioned by a define; a field of any other type fails with the struct and the field named."""
    import pytest
    import build as omnipq_build
    inc = tmp_path / "include"
    inc.mkdir()
    monkeypatch.setattr(omnipq_build, "REPO", str(tmp_path))
    (inc / "a.h").write_text("#ifndef OMNIPQ_A_H\n#define OMNIPQ_A_H\n#define OMNIPQ_N 3   /* x */\n#define OMNIPQ_FLAG 2u\n"
                             "typedef struct omnipq_tag {\n  int a, b;  /* two */\n  const float *x, *y[OMNIPQ_N];\n"
                             "  unsigned long long w; long long v; float f[2]; const void *q;\n} omnipq_rec;\n#endif\n")
    assert omnipq_build.abi_records() == ("define OMNIPQ_FLAG 2\ndefine OMNIPQ_N 3\n"
                                          "struct omnipq_rec a:i b:i x:p y:p*3 w:L v:l f:f*2 q:p\n")
    for body, field in (("int a; short bad_one;", "bad_one"), ("int a; struct { int c; } bad_two;", "bad_two"),
                        ("omnipq_rec bad_three;", "bad_three"), ("float bad_four[OMNIPQ_UNKNOWN];", "bad_four"),
                        ("int a, bad_five[2][2];", "bad_five")):
        (inc / "b.h").write_text("typedef struct { " + body + " } omnipq_worse;\n")
        with pytest.raises(RuntimeError, match=f"omnipq_worse.*{field}"):
            omnipq_build.abi_records()


def test_layout_checks_refuse_a_layout_the_text_does_not_state(built_lib, tmp_path, monkeypatch):
    """The static_asserts build.py writes from the reported text (compiled into csrc/capi.hip of both libraries) hold for the
    header they were written from and stop the compiler once two fields of different width change places.  Host compiler
    only: the translation unit has no device code."""
    import subprocess
    import build as omnipq_build
    inc = tmp_path / "include"
    inc.mkdir()
    monkeypatch.setattr(omnipq_build, "REPO", str(tmp_path))
    (inc / "a.h").write_text("typedef struct { int n; const float *x; float w; } omnipq_rec;\n")
    checks = omnipq_build.layout_checks(omnipq_build.abi_records())
    assert checks.count("static_assert(") == 4 and "sizeof(omnipq_rec) == 24" in checks
    assert "offsetof(omnipq_rec, x) == 8" in checks and "offsetof(omnipq_rec, w) == 16" in checks
    (tmp_path / "checks.inc").write_text(checks)
    (tmp_path / "tu.cpp").write_text('#include <stddef.h>\n#include "include/a.h"\n#include "checks.inc"\nint main() { return 0; }\n')
    cmd = [omnipq_build.hipcc(), "-x", "c++", "-std=c++17", "-fsyntax-only", "tu.cpp"]
    done = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    (inc / "a.h").write_text("typedef struct { const float *x; int n; float w; } omnipq_rec;\n")
    done = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert done.returncode != 0 and "omnipq_rec.x: offset" in done.stderr and "omnipq_rec.n: offset" in done.stderr


_FIELD_CTYPE = {"i": ctypes.c_int, "u": ctypes.c_uint, "l": ctypes.c_longlong, "L": ctypes.c_ulonglong, "f": ctypes.c_float,
                "d": ctypes.c_double, "p": ctypes.c_void_p}


def test_library_reports_the_structs_and_defines_its_headers_declare(built_lib):
    """Every `typedef struct` and every valued `#define OMNIPQ_*` of include/*.h is reported by both libraries as the headers
    state it (read by tests/capi.py, not by the build), nothing else is reported, and the binding's struct() / const() return
    exactly these.  This is the one guard of every descriptor and limit the Python modules take from the library."""
    import pytest
    defines, structs = capi.declared_records()
    assert len(structs) == 12 and len(defines) == 29 and len(structs["omnipq_asm_out"]) == 31
    assert defines["OMNIPQ_MT_MAX_K"] == 512 and defines["OMNIPQ_ABI_VERSION"] == 5
    assert structs["omnipq_pc_desc"][-1] == ("not_solid", "L", None) and structs["omnipq_mt_grads"][0] == ("center", "p", 8)
    for path in both(built_lib):
        got_defines, got_structs = capi.reported_records(ctypes.CDLL(path))
        assert got_defines == defines, path
        assert sorted(set(got_structs) ^ set(structs)) == [], path
        assert {n: got_structs[n] for n in structs if got_structs[n] != structs[n]} == {}, path
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    assert {name: ext.const(name) for name in defines} == defines
    for name, fields in structs.items():
        cls = ext.struct(name)
        assert cls is ext.struct(name) and issubclass(cls, ctypes.Structure)
        assert cls._fields_ == [(f, _FIELD_CTYPE[t] * n if n else _FIELD_CTYPE[t]) for f, t, n in fields], name
    assert ctypes.sizeof(ext.struct("omnipq_mt_desc")) == 24 + 17 * 8 * 8 + 5 * 8
    assert ctypes.sizeof(ext.struct("omnipq_mt_grads")) == 8 * 8 * 8
    pc = ext.struct("omnipq_pc_desc")
    assert pc._fields_[-1] == ("not_solid", ctypes.c_ulonglong)
    assert pc.not_solid.offset == ctypes.sizeof(pc) - 8 == max(getattr(pc, f).offset for f, _ in pc._fields_)
    for ask, name in ((ext.const, "OMNIPQ_MT_MAX_Q"), (ext.struct, "omnipq_mt_descr"), (ext.const, "omnipq_mt_desc"),
                      (ext.struct, "OMNIPQ_MT_MAX_K")):
        with pytest.raises(KeyError, match="reports no"):
            ask(name)


def test_binding_refuses_miscounted_and_mistyped_calls(built_lib):
    """Through the binding a call one argument short or one long raises TypeError, a pointer where the header says `int`
    raises ctypes.ArgumentError, and a plain Python int arrives whole in a `long long` parameter -- through an untyped handle
    it is cut to a C int (1 << 45 -> 0) and omnipq_copy_probe answers OMNIPQ_OK.  Nothing here reaches a device: every call
    is refused by ctypes or by the entry point's own validation."""
    import pytest
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    EINVAL = 10001
    p = ctypes.c_void_p(0x1000)                       # never dereferenced
    good = (0, 128, 32, p, 32, p, 32, p, 128, None, None)      # omnipq_gemm_nt_e16 on zero rows: a no-op that succeeds
    assert ext._lib.omnipq_gemm_nt_e16(*good) == 0
    with pytest.raises(TypeError, match="omnipq_gemm_nt_e16"):
        ext._lib.omnipq_gemm_nt_e16(*good[:-1])
    with pytest.raises(TypeError, match="omnipq_gemm_nt_e16"):
        ext._lib.omnipq_gemm_nt_e16(*good, None)
    with pytest.raises(TypeError):
        ext._lib0.omnipq_copy_probe(p, p, 16)                   # a bare library function: ctypes counts the missing one
    with pytest.raises(ctypes.ArgumentError):
        ext._lib.omnipq_gemm_nt_e16(p, 128, 32, p, 32, p, 32, p, 128, None, None)
    with pytest.raises(ctypes.ArgumentError):
        ext._lib0.omnipq_ball_query(1, 16, 4, 0.2, p, p, p, p, None)          # nsample is an int
    assert capi.lib().omnipq_copy_probe(p, p, 1 << 45, None) == 0                # the bug class: bytes arrived as 0
    assert ext._lib.omnipq_copy_probe(p, p, 1 << 45, None) == EINVAL
    assert ext._lib0.omnipq_copy_probe(p, p, 1 << 45, None) == EINVAL
    assert ext._lib0.omnipq_copy_probe(p, p, ctypes.c_longlong(1 << 45), None) == EINVAL     # a wrapped scalar still works


def test_host_helpers_without_gpu(built_lib):
    from oracle import oracle_ext
    lib = capi.lib()
    assert lib.omnipq_abi_version() == 5
    assert b"invalid" in lib.omnipq_error_string(10001)
    # the FPS tie geometry must agree between library, oracle and the reference's formula
    for n in list(range(1, 70)) + [100, 127, 128, 255, 256, 511, 512, 513, 1000, 1024, 2048, 4096, 8192,
                                   40000, 50000, 80000, 1 << 20]:
        assert lib.omnipq_opt_n_threads(n) == oracle_ext.opt_n_threads(n), n
    assert lib.omnipq_opt_n_threads(40000) == 512 and lib.omnipq_opt_n_threads(100) == 64


def test_argument_validation_needs_no_gpu(built_lib):
    """Every entry point rejects malformed arguments with OMNIPQ_EINVAL / OMNIPQ_ETOOLARGE BEFORE it touches the
    device (the reference's wrappers `exit(-1)` from inside the launch, cuda_utils.h:35-44).  Pointers below
    are never dereferenced: validation comes first."""
    lib = capi.lib()
    EINVAL, ETOOLARGE = 10001, 10002
    p = ctypes.c_void_p(0x1000)                       # "some non-null pointer"
    null = ctypes.c_void_p(0)
    f = ctypes.c_float
    ll = ctypes.c_longlong
    strides = (ll * 8)(288, 2304, 288, 2304, 288, 2304, 288, 2304)
    # attention: head dim not a multiple of 4 / too wide, dropout outside [0, 1), problem beyond 32-bit indexing
    assert lib.omnipq_attn_fwd(8, 8, 256, 256, 37, p, p, p, p, strides, p, f(0.0), null, 0, null) == EINVAL
    assert lib.omnipq_attn_fwd(8, 8, 256, 256, 52, p, p, p, p, strides, p, f(0.0), null, 0, null) == EINVAL
    assert lib.omnipq_attn_fwd(8, 8, 256, 256, 36, p, p, p, p, strides, p, f(1.0), p, 0, null) == EINVAL
    assert lib.omnipq_attn_fwd(8, 8, 256, 256, 36, p, p, p, p, strides, p, f(0.1), null, 0, null) == EINVAL   # no seed
    assert lib.omnipq_attn_fwd(64, 16, 4096, 4096, 36, p, p, p, p, strides, p, f(0.0), null, 0, null) == ETOOLARGE
    # a negative token stride has no extent to bound the kernels' reads by (att_rsrc: num_records would be negative, which the
    # hardware takes for no bound at all): refused by forward and backward, for every tensor, before any launch
    good = [288, 2304, 288, 2304, 288, 2304, 288, 2304]
    ggood = [288, 2304, 288, 2304, 288, 2304]

    def bwd(st, gst):
        return lib.omnipq_attn_bwd(8, 8, 256, 256, 36, p, p, p, p, p, (ll * 8)(*st), p, p, p, p, p, (ll * 6)(*gst), f(0.0),
                                   null, 0, null)

    for i in (0, 2, 4, 6):
        for bad in (-288, -4):
            st = list(good)
            st[i] = bad
            assert lib.omnipq_attn_fwd(8, 8, 256, 256, 36, p, p, p, p, (ll * 8)(*st), p, f(0.0), null, 0, null) == EINVAL, i
            assert bwd(st, ggood) == EINVAL, i
    for i in (0, 2, 4):
        for bad in (-288, -4):
            gst = list(ggood)
            gst[i] = bad
            assert bwd(good, gst) == EINVAL, i
    assert bwd(good, [288, 2304, 288, 2304, 290, 2304]) == EINVAL                      # the rules that were there stay
    assert bwd(good, [288, 2304, 1 << 30, 2304, 288, 2304]) == ETOOLARGE
    assert lib.omnipq_attn_fwd(8, 8, 256, 256, 36, p, p, p, p, (ll * 8)(1 << 30, 2304, 288, 2304, 288, 2304, 288, 2304), p,
                               f(0.0), null, 0, null) == ETOOLARGE
    # GEMMs: contraction length must be a multiple of the K step, leading dimensions of 8
    assert lib.omnipq_gemm_nt_e16(128, 128, 33, p, 40, p, 40, p, 128, null, null) == EINVAL
    assert lib.omnipq_gemm_nt_e16_stats(128, 128, 32, p, 32, p, 32, p, 128, null, null, null, null, null) == EINVAL  # no sums
    assert lib.omnipq_gemm_tn_e16(100, 128, 64, p, 100, p, 128, p, p, null, null) == EINVAL                      # M % 8
    lib.omnipq_gemm_nt_stats_workspace_floats.restype = ll
    assert lib.omnipq_gemm_nt_stats_workspace_floats(64 * 128, 256) == 0
    assert lib.omnipq_gemm_nt_stats_workspace_floats(64 * 128 + 1, 256) == 65 * 2 * 256
    # row kernels
    assert lib.omnipq_add_dropout_layernorm(ll(10), 290, p, p, p, p, f(1e-5), f(0.0), null, 0, p, p, null, null, p, p,
                                            null) == EINVAL                                                   # C % 4
    assert lib.omnipq_add_dropout_layernorm(ll(10), 288, p, p, p, p, f(1e-5), f(0.0), null, 0, p, p, p, null, p, p,
                                            null) == EINVAL                                     # pe without its output
    assert lib.omnipq_relu_dropout(ll(10), p, f(0.0), null, 0, null) == EINVAL                                 # n % 4
    assert lib.omnipq_interp_rows(2, 10, 5, 64, p, p, p, p, 64, 8, null) == EINVAL             # columns do not fit
    assert lib.omnipq_place_rows(ll(10), 64, p, p, 100, 0, null) == EINVAL                               # pitch % 8
    assert lib.omnipq_colsum_f32(ll(10), 12, p, p, null) == EINVAL
    # loss helper: more views than the kernel-argument table holds
    ptrs = (ctypes.c_void_p * 73)(*([0x1000] * 73))
    ones = (ctypes.c_int * (73 * 4))(*([1] * 73 * 4))
    flags = (ctypes.c_int * 73)()
    assert lib.omnipq_sum_of_means(73, ptrs, ones, ones, flags, p, null) == EINVAL
    # zero-sized problems are no-ops that succeed without a device
    assert lib.omnipq_gemm_nt_e16(0, 128, 32, p, 32, p, 32, p, 128, null, null) == 0
    assert lib.omnipq_interp_rows(0, 10, 5, 64, p, p, p, p, 64, 0, null) == 0
    assert lib.omnipq_relu_dropout(ll(0), p, f(0.0), null, 0, null) == 0


def test_last_layer_route_rejects_the_shapes_it_does_not_compute(built_lib):
    """The entry points of a planned stage's last-layer backward without dY3 (include/omnipq_sa.h) check the
    preconditions their header states before they touch the device: C2 and C3 multiples of 128 (all four), the stage's plan with
    their row count (dz_bnbwd, tn_dz), more than 64 row tiles (dz_bnbwd, the no-store forward), nsample a power of two."""
    import sa_fused
    lib = capi.lib()
    EINVAL = 10001
    p = ctypes.c_void_p(0x1000)                       # never dereferenced: every call below is rejected first
    null = ctypes.c_void_p(0)
    ll, d, f = ctypes.c_longlong, ctypes.c_double, ctypes.c_float
    P, S = 10240, 32

    def plan(rows):
        return ctypes.pointer(sa_fused.RowPlanArg(0x1000, 0x1000, 0x1000, rows, 8, None))

    def prep(C3, C2, hot=null, g=null):
        return lib.omnipq_sa_last_bwd_prep(ll(P // S), C3, C2, p, d(float(P)), p, p, p, g, g, g, p, C3, hot, p, C2 + 32, p, p,
                                           null, null)

    def dz(M, N, C3, nsample=S, pl=None):
        pl = plan(M) if pl is None else pl
        return lib.omnipq_gemm_nt_e16_dz_bnbwd(M, N, C3, p, N, p, N + 32, p, C3, p, p, nsample, p, N, p, p, p, p, p, p, null,
                                               pl, null)

    def tn(C3, N, P_, nsample=S, pl=None):
        pl = plan(P_) if pl is None else pl
        slabs, off = ctypes.c_int(0), ctypes.c_longlong(0)
        return lib.omnipq_gemm_tn_dz(C3, N, P_, p, N, null, null, p, p, nsample, p, ctypes.byref(slabs), ctypes.byref(off), pl,
                                     null)

    def combine(C3, C2):
        return lib.omnipq_sa_last_wgrad_combine(C3, C2, p, p, 1, C3 + C2, p, p, p, C2, p, C2, 0, null)

    for C3, C2 in ((192, 128), (256, 160), (64, 128), (128, 96), (256, 32)):
        assert prep(C3, C2) == EINVAL, ("prep", C3, C2)
        assert dz(P, C2, C3) == EINVAL, ("dz_bnbwd", C3, C2)
        assert tn(C3, C2, P) == EINVAL, ("tn_dz", C3, C2)
        assert combine(C3, C2) == EINVAL, ("combine", C3, C2)
    assert prep(256, 128, hot=p) == EINVAL                                            # hot without g_out / out_pm / arg
    assert dz(P, 128, 256, nsample=48) == EINVAL and tn(256, 128, P, nsample=48) == EINVAL      # nsample not a power of two
    assert dz(P, 128, 256, nsample=4) == EINVAL and tn(256, 128, P, nsample=4) == EINVAL
    assert dz(P, 128, 256, pl=null) == EINVAL and tn(256, 128, P, pl=null) == EINVAL            # no plan
    assert dz(P, 128, 256, pl=plan(P + 128)) == EINVAL                                  # a plan of another row count
    assert tn(256, 128, P, pl=plan(P - 128)) == EINVAL                                  # rows != P
    assert dz(8192, 128, 256) == EINVAL                                                 # 64 row tiles: m_tiles <= 64
    # the no-store forward (C = NULL) on 64 row tiles
    assert lib.omnipq_gemm_nt_e16_bnaffine_pool(8192, 256, 128, p, 128, p, d(8192.0), p, p, f(1e-5), f(0.1), null, null, null,
                                                p, p, p, p, p, 128, null, 256, null, p, p, 8, p, p, p, p, plan(8192),
                                                null) == EINVAL
    # ... and the host sends the route nothing else (sa_fused.last_no_dy_ok)
    import types
    pl = types.SimpleNamespace(unit_src=object())
    assert sa_fused.last_no_dy_ok(pl, 3, P, 128, 256, S, True)
    assert not sa_fused.last_no_dy_ok(pl, 3, P, 160, 256, S, True) and not sa_fused.last_no_dy_ok(pl, 3, P, 128, 192, S, True)
    assert not sa_fused.last_no_dy_ok(pl, 3, 8192, 128, 256, S, True)
